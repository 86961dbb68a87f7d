"""Seeded synthetic inputs: there is no dataset and no network, so the tests and bench.py
generate EuRoC-shaped images here.  Pure numpy; deterministic for a given seed."""
import numpy as np


def _value_noise(rng, h, w, cell):
    gh, gw = h // cell + 2, w // cell + 2
    g = rng.random((gh, gw)).astype(np.float32)
    ys = np.arange(h, dtype=np.float32) / cell
    xs = np.arange(w, dtype=np.float32) / cell
    y0 = ys.astype(np.int32); x0 = xs.astype(np.int32)
    fy = (ys - y0)[:, None]; fx = (xs - x0)[None, :]
    a = g[y0][:, x0]; b = g[y0][:, x0 + 1]; c = g[y0 + 1][:, x0]; d = g[y0 + 1][:, x0 + 1]
    return (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy


def make_image(w=752, h=480, seed=0, n_shapes=None, noise_sigma=2.0):
    """u8 HxW image: 3 octaves of value noise + random rectangles/discs + Gaussian pixel noise."""
    rng = np.random.default_rng(0x4D0B + seed)
    img = 96 * _value_noise(rng, h, w, 64) + 64 * _value_noise(rng, h, w, 16) + 32 * _value_noise(rng, h, w, 4)
    img += 20
    if n_shapes is None:
        n_shapes = int(400 * (w * h) / 360960)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(n_shapes):
        cx, cy = rng.integers(0, w), rng.integers(0, h)
        s = int(rng.integers(3, 40))
        grey = float(rng.integers(0, 256))
        kind = rng.integers(0, 3)
        x0, x1 = max(cx - s, 0), min(cx + s + 1, w)
        y0, y1 = max(cy - s, 0), min(cy + s + 1, h)
        if x1 <= x0 or y1 <= y0:
            continue
        sub = img[y0:y1, x0:x1]
        if kind == 0:
            sub[:] = grey
        elif kind == 1:
            m = (xx[y0:y1, x0:x1] - cx) ** 2 + (yy[y0:y1, x0:x1] - cy) ** 2 <= s * s
            sub[m] = grey
        else:  # rotated rectangle
            th = rng.random() * np.pi
            u = (xx[y0:y1, x0:x1] - cx) * np.cos(th) + (yy[y0:y1, x0:x1] - cy) * np.sin(th)
            v = -(xx[y0:y1, x0:x1] - cx) * np.sin(th) + (yy[y0:y1, x0:x1] - cy) * np.cos(th)
            m = (np.abs(u) <= s * 0.8) & (np.abs(v) <= s * 0.4)
            sub[m] = grey
    img += rng.normal(0, noise_sigma, size=img.shape)
    return np.ascontiguousarray(np.clip(np.rint(img), 0, 255).astype(np.uint8))


def make_stereo_pair(w=752, h=480, seed=0, dmin=2.0, dmax=60.0):
    """(left, right): right = left warped by a smooth horizontal disparity field d(x,y) in [dmin, dmax]
    (left pixel (x,y) appears at (x-d, y) in the right image), plus independent pixel noise."""
    left = make_image(w, h, seed)
    rng = np.random.default_rng(0x57E0 + seed)
    d = dmin + (dmax - dmin) * _value_noise(rng, h, w, 128)
    xs = np.arange(w, dtype=np.float32)[None, :] + d  # right(x) samples left(x + d)
    x0 = np.clip(np.floor(xs).astype(np.int32), 0, w - 1)
    x1 = np.clip(x0 + 1, 0, w - 1)
    f = xs - np.floor(xs)
    rows = np.arange(h)[:, None]
    L = left.astype(np.float32)
    right = L[rows, x0] * (1 - f) + L[rows, x1] * f + rng.normal(0, 1.0, size=L.shape)
    return left, np.ascontiguousarray(np.clip(np.rint(right), 0, 255).astype(np.uint8))


def shift_image(img, dx, dy):
    """Integer global shift with edge replication (feeds the frame-to-frame matchers)."""
    h, w = img.shape
    ys = np.clip(np.arange(h) - dy, 0, h - 1)
    xs = np.clip(np.arange(w) - dx, 0, w - 1)
    return np.ascontiguousarray(img[ys][:, xs])


def make_vocabulary(k=10, L=6, seed=0):
    """Synthetic DBoW2-shaped ORB vocabulary (the real ORBvoc.txt is a missing blob, SURVEY.md finding 3):
    complete k-ary tree of depth L in level order (node 0 = root, children of n = k*n+1 .. k*n+k), each child
    descriptor = parent descriptor with a level-dependent fraction of random bits flipped.
    Returns (nodeDesc [nnodes, 32] u8, firstChild [nnodes] i32, -1 for leaves)."""
    rng = np.random.default_rng(0xB0 + seed)
    nn = (k ** (L + 1) - 1) // (k - 1)
    desc = np.zeros((nn, 32), np.uint8)
    first = np.full(nn, -1, np.int32)
    desc[0] = rng.integers(0, 256, 32, dtype=np.uint8)
    start, cnt = 0, 1
    for lvl in range(L):
        parents = np.arange(start, start + cnt)
        first[parents] = k * parents + 1
        p = 0.5 / (lvl + 1.5)
        child_ids = (k * parents[:, None] + 1 + np.arange(k)[None, :]).reshape(-1)
        flips = np.packbits(rng.random((len(child_ids), 256)) < p, axis=1)
        desc[child_ids] = np.repeat(desc[parents], k, axis=0) ^ flips
        start, cnt = start + cnt, cnt * k
    return desc, first


# ---- synthetic geometry for the optimisers ------------------------------------------------
EUROC_CAM = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, bf=458.654 * 0.11)


def _quat_from_rotvec(r):
    th = np.linalg.norm(r)
    if th < 1e-12:
        return np.array([0, 0, 0, 1.0])
    a = r / th
    return np.concatenate([a * np.sin(th / 2), [np.cos(th / 2)]])


def _quat_mul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def _quat_rot(q, v):
    u, w = q[:3], q[3]
    uv = 2 * np.cross(u, v)
    return v + w * uv + np.cross(u, uv)


def _project(pose, X, cam):
    """pose = (qx,qy,qz,qw,tx,ty,tz) world->camera; returns (u, v, uRight, z)."""
    Xc = np.array([_quat_rot(pose[:4], x) for x in X]) + pose[4:]
    z = Xc[:, 2]
    u = cam["fx"] * Xc[:, 0] / z + cam["cx"]
    v = cam["fy"] * Xc[:, 1] / z + cam["cy"]
    return u, v, u - cam["bf"] / z, z


def make_pose_problem(n=600, seed=0, outlier_frac=0.1, mono_frac=0.3, rot_deg=2.0, trans=0.05, cam=EUROC_CAM):
    """One PoseOptimization input: n features, ~all with a MapPoint, stereo/mono mix, gross outliers, perturbed
    initial pose.  Returns dict of float32 arrays + the true pose."""
    rng = np.random.default_rng(0x9050 + seed)
    true = np.concatenate([_quat_from_rotvec(rng.normal(0, 0.1, 3)), rng.normal(0, 0.3, 3)])
    # points in front of the camera: sample camera-frame points and map them to the world
    Xc = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(2, 10, n)], 1)
    qinv = true[:4] * np.array([-1, -1, -1, 1])
    Xw = np.array([_quat_rot(qinv, x - true[4:]) for x in Xc])
    u, v, ur, z = _project(true, Xw, cam)
    octave = rng.integers(0, 8, n)
    sigma = 1.2 ** octave
    u = u + rng.normal(0, 1, n) * sigma; v = v + rng.normal(0, 1, n) * sigma; ur = ur + rng.normal(0, 1, n) * sigma
    out = rng.random(n) < outlier_frac
    u[out] += rng.choice([-1, 1], out.sum()) * rng.uniform(15, 40, out.sum())
    v[out] += rng.choice([-1, 1], out.sum()) * rng.uniform(15, 40, out.sum())
    mono = rng.random(n) < mono_frac
    ur[mono] = -1
    has = (rng.random(n) < 0.9).astype(np.uint8)
    dq = _quat_from_rotvec(rng.normal(0, 1, 3) / np.sqrt(3) * np.deg2rad(rot_deg))
    init = np.concatenate([_quat_mul(dq, true[:4]), _quat_rot(dq, true[4:]) + rng.normal(0, trans, 3)])
    return dict(hasMP=has, obs=np.stack([u, v, ur], 1).astype(np.float32), invSigma2=(1.0 / sigma ** 2).astype(np.float32),
                Xw=Xw.astype(np.float32), pose0=init.astype(np.float32), true=true, outlier_truth=out, cam=cam)


def make_ba_problem(n_free=20, n_fixed=6, n_points=3000, seed=0, outlier_frac=0.05, mono_frac=0.15, cam=EUROC_CAM):
    """LocalBundleAdjustment input shaped like BASELINE config 5: n_free + n_fixed keyframes on an arc looking at
    a point slab, each point observed by 4-10 keyframes."""
    rng = np.random.default_rng(0xBA00 + seed)
    nkf = n_free + n_fixed
    poses = []
    for i in range(nkf):
        ang = (i / max(nkf - 1, 1) - 0.5) * 0.5
        c = np.array([2.0 * np.sin(ang) * 2, rng.normal(0, 0.05), -2.0 * (1 - np.cos(ang))])   # camera centre
        q_wc = _quat_from_rotvec(np.array([0, -ang * 0.8, 0]) + rng.normal(0, 0.01, 3))      # camera->world
        q_cw = q_wc * np.array([-1, -1, -1, 1])
        poses.append(np.concatenate([q_cw, -_quat_rot(q_cw, c)]))
    poses = np.array(poses)
    X = np.stack([rng.uniform(-3, 3, n_points), rng.uniform(-2, 2, n_points), rng.uniform(3, 10, n_points)], 1)
    eKF, eMP, eObs, eInv = [], [], [], []
    for j in range(n_points):
        k = int(rng.integers(4, 11))
        kfs = rng.choice(nkf, size=min(k, nkf), replace=False)
        u, v, ur, z = _project_many(poses[kfs], X[j], cam)
        for a, kf in enumerate(kfs):
            if z[a] <= 0.5 or not (0 <= u[a] < 752 and 0 <= v[a] < 480):
                continue
            octv = int(rng.integers(0, 8)); s = 1.2 ** octv
            o = np.array([u[a], v[a], ur[a]]) + rng.normal(0, 1, 3) * s
            if rng.random() < outlier_frac:
                o[:2] += rng.choice([-1, 1], 2) * rng.uniform(15, 30, 2)
            if rng.random() < mono_frac:
                o[2] = -1
            eKF.append(kf); eMP.append(j); eObs.append(o); eInv.append(1.0 / s ** 2)
    fixed = np.zeros(nkf, np.uint8); fixed[n_free:] = 1
    pose0 = poses.copy()
    for i in range(n_free):
        dq = _quat_from_rotvec(rng.normal(0, 1, 3) / np.sqrt(3) * np.deg2rad(2.0))
        pose0[i] = np.concatenate([_quat_mul(dq, poses[i][:4]), _quat_rot(dq, poses[i][4:]) + rng.normal(0, 0.05, 3)])
    X0 = X + rng.normal(0, 0.05, X.shape)
    return dict(kfPose=pose0.astype(np.float32), kfFixed=fixed, mpPos=X0.astype(np.float32),
                eKF=np.array(eKF, np.int32), eMP=np.array(eMP, np.int32), eObs=np.array(eObs, np.float32),
                eInvSigma2=np.array(eInv, np.float32), true_poses=poses, true_points=X, cam=cam)


def _project_many(poses, x, cam):
    Xc = np.array([_quat_rot(p[:4], x) + p[4:] for p in poses])
    z = Xc[:, 2]
    u = cam["fx"] * Xc[:, 0] / z + cam["cx"]
    v = cam["fy"] * Xc[:, 1] / z + cam["cy"]
    return u, v, u - cam["bf"] / z, z


# ---- fisheye rig (TUM-VI, Examples/Stereo/TUM-VI.yaml) -------------------------------------------------------
TUMVI_CAM_L = np.array([190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504,
                        0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182], np.float32)
TUMVI_CAM_R = np.array([190.44236969414825, 190.4344384721956, 252.59949716835982, 254.91723064636983,
                        0.0034003170790442797, 0.001766278153469831, -0.00266312569781606, 0.0003299517423931039], np.float32)
TUMVI_T_C1_C2 = np.array([[0.999999445773493, 0.000791687752817, 0.000694034010224, 0.101063427414194],
                          [-0.000823363992158, 0.998899461915674, 0.046895490788700, 0.001946204678584],
                          [-0.000656143613644, -0.046896036240590, 0.998899560146304, 0.001015350132563],
                          [0, 0, 0, 1.0]])   # Stereo.T_c1_c2 = Tlr (right-camera coordinates -> left-camera coordinates)


def kb8_project(cam, X):
    """KannalaBrandt8::project in float64 numpy (reference formula) for an [n, 3] array."""
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    th = np.arctan2(np.sqrt(x * x + y * y), z); psi = np.arctan2(y, x)
    r = th + cam[4] * th ** 3 + cam[5] * th ** 5 + cam[6] * th ** 7 + cam[7] * th ** 9
    return np.stack([cam[0] * r * np.cos(psi) + cam[2], cam[1] * r * np.sin(psi) + cam[3]], 1)


def _quat_from_R(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def make_fisheye_features(n_pairs=600, n_mono=80, n_distract=150, seed=0):
    """Synthetic fisheye stereo feature sets (no images): n_pairs 3-D points seen by both KB8 cameras with matching
    descriptors (a few bits flipped), mono-area features in front of the arrays, unmatched distractors behind."""
    rng = np.random.default_rng(0xF15E + seed)
    Tlr = TUMVI_T_C1_C2
    Trl = np.linalg.inv(Tlr)
    X = np.stack([rng.uniform(-4, 4, n_pairs), rng.uniform(-3, 3, n_pairs), rng.uniform(0.8, 8, n_pairs)], 1)
    uvL = kb8_project(TUMVI_CAM_L, X) + rng.normal(0, 0.2, (n_pairs, 2))
    Xr = X @ Trl[:3, :3].T + Trl[:3, 3]
    uvR = kb8_project(TUMVI_CAM_R, Xr) + rng.normal(0, 0.2, (n_pairs, 2))
    ok = (uvL > 20).all(1) & (uvL < 492).all(1) & (uvR > 20).all(1) & (uvR < 492).all(1) & (Xr[:, 2] > 0.3)
    uvL, uvR = uvL[ok], uvR[ok]
    m = len(uvL)
    base = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    flip = np.packbits(rng.random((m, 256)) < 0.03, axis=1)
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

    def side(uv, desc, nm, nd):
        n = nm + len(uv) + nd
        k = np.zeros(n, dt); d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        k["x"] = rng.uniform(20, 492, n); k["y"] = rng.uniform(20, 492, n)
        k["octave"] = rng.integers(0, 8, n); k["size"] = 31; k["angle"] = rng.uniform(0, 360, n); k["class_id"] = -1
        perm = rng.permutation(len(uv))
        k["x"][nm:nm + len(uv)] = uv[perm, 0]; k["y"][nm:nm + len(uv)] = uv[perm, 1]
        d[nm:nm + len(uv)] = desc[perm]
        return k, d, nm

    kL, dL, monoL = side(uvL, base, n_mono, n_distract)
    kR, dR, monoR = side(uvR, base ^ flip, n_mono // 2, n_distract)
    return dict(kL=kL, dL=dL, monoL=monoL, kR=kR, dR=dR, monoR=monoR, Rlr=Tlr[:3, :3].astype(np.float32),
                tlr=Tlr[:3, 3].astype(np.float32), camL=TUMVI_CAM_L, camR=TUMVI_CAM_R)


def make_pose_problem_fisheye(n_left=400, n_right=300, seed=0, outlier_frac=0.1, rot_deg=2.0, trans=0.05):
    """PoseOptimization input for the fisheye rig: left-camera and right-camera observations of map points."""
    rng = np.random.default_rng(0xF0E5 + seed)
    Trl_m = np.linalg.inv(TUMVI_T_C1_C2)
    true = np.concatenate([_quat_from_rotvec(rng.normal(0, 0.1, 3)), rng.normal(0, 0.3, 3)])
    n = n_left + n_right
    Xc = np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(1, 8, n)], 1)
    qinv = true[:4] * np.array([-1, -1, -1, 1])
    Xw = np.array([_quat_rot(qinv, x - true[4:]) for x in Xc])
    uv = np.zeros((n, 2))
    uv[:n_left] = kb8_project(TUMVI_CAM_L, Xc[:n_left])
    Xr = Xc[n_left:] @ Trl_m[:3, :3].T + Trl_m[:3, 3]
    uv[n_left:] = kb8_project(TUMVI_CAM_R, Xr)
    octave = rng.integers(0, 8, n); sigma = 1.2 ** octave
    uv += rng.normal(0, 0.5, (n, 2)) * sigma[:, None]
    out = rng.random(n) < outlier_frac
    uv[out] += rng.choice([-1, 1], (out.sum(), 2)) * rng.uniform(15, 40, (out.sum(), 2))
    dq = _quat_from_rotvec(rng.normal(0, 1, 3) / np.sqrt(3) * np.deg2rad(rot_deg))
    init = np.concatenate([_quat_mul(dq, true[:4]), _quat_rot(dq, true[4:]) + rng.normal(0, trans, 3)])
    obs = np.concatenate([uv, np.zeros((n, 1))], 1).astype(np.float32)
    Trl7 = np.concatenate([_quat_from_R(Trl_m[:3, :3]), Trl_m[:3, 3]]).astype(np.float32)
    return dict(hasMP=(rng.random(n) < 0.92).astype(np.uint8), obs=obs, invSigma2=(1 / sigma ** 2).astype(np.float32),
                Xw=Xw.astype(np.float32), pose0=init.astype(np.float32), true=true, Nleft=n_left, camL=TUMVI_CAM_L, camR=TUMVI_CAM_R,
                Trl=Trl7)


def make_ba_problem_fisheye(n_free=10, n_fixed=4, n_points=1500, seed=0, outlier_frac=0.05, right_frac=0.45):
    """LocalBundleAdjustment input on the TUM-VI KannalaBrandt8 rig: left-camera observations (EdgeSE3ProjectXYZ) and
    right-camera observations behind Trl (EdgeSE3ProjectXYZToBody)."""
    rng = np.random.default_rng(0xFBA0 + seed)
    Trl_m = np.linalg.inv(TUMVI_T_C1_C2)
    nkf = n_free + n_fixed
    poses = []
    for i in range(nkf):
        ang = (i / max(nkf - 1, 1) - 0.5) * 0.5
        c = np.array([2.0 * np.sin(ang) * 2, rng.normal(0, 0.05), -2.0 * (1 - np.cos(ang))])
        q_wc = _quat_from_rotvec(np.array([0, -ang * 0.8, 0]) + rng.normal(0, 0.01, 3))
        q_cw = q_wc * np.array([-1, -1, -1, 1])
        poses.append(np.concatenate([q_cw, -_quat_rot(q_cw, c)]))
    poses = np.array(poses)
    X = np.stack([rng.uniform(-3, 3, n_points), rng.uniform(-2, 2, n_points), rng.uniform(2, 8, n_points)], 1)
    eKF, eMP, eObs, eInv, eRight = [], [], [], [], []
    for j in range(n_points):
        kfs = rng.choice(nkf, size=min(int(rng.integers(4, 9)), nkf), replace=False)
        for kf in kfs:
            Xc = _quat_rot(poses[kf][:4], X[j]) + poses[kf][4:]
            for right in (0, 1):
                if right and rng.random() > right_frac:
                    continue
                Xs = Trl_m[:3, :3] @ Xc + Trl_m[:3, 3] if right else Xc
                if Xs[2] <= 0.4:
                    continue
                uv = kb8_project(TUMVI_CAM_R if right else TUMVI_CAM_L, Xs[None])[0]
                if not (5 < uv[0] < 507 and 5 < uv[1] < 507):
                    continue
                octv = int(rng.integers(0, 8)); sg = 1.2 ** octv
                o = uv + rng.normal(0, 0.7, 2) * sg
                if rng.random() < outlier_frac:
                    o += rng.choice([-1, 1], 2) * rng.uniform(15, 30, 2)
                eKF.append(kf); eMP.append(j); eObs.append(o); eInv.append(1.0 / sg ** 2); eRight.append(right)
    fixed = np.zeros(nkf, np.uint8); fixed[n_free:] = 1
    pose0 = poses.copy()
    for i in range(n_free):
        dq = _quat_from_rotvec(rng.normal(0, 1, 3) / np.sqrt(3) * np.deg2rad(1.5))
        pose0[i] = np.concatenate([_quat_mul(dq, poses[i][:4]), _quat_rot(dq, poses[i][4:]) + rng.normal(0, 0.03, 3)])
    X0 = X + rng.normal(0, 0.04, X.shape)
    Trl7 = np.concatenate([_quat_from_R(Trl_m[:3, :3]), Trl_m[:3, 3]]).astype(np.float32)
    return dict(kfPose=pose0.astype(np.float32), kfFixed=fixed, mpPos=X0.astype(np.float32), eKF=np.array(eKF, np.int32),
                eMP=np.array(eMP, np.int32), eObs=np.array(eObs, np.float32), eInvSigma2=np.array(eInv, np.float32),
                eRight=np.array(eRight, np.uint8), camL=TUMVI_CAM_L, camR=TUMVI_CAM_R, Trl=Trl7, true_poses=poses, true_points=X)


# ---- visual-inertial tracking (PoseInertialOptimizationLastKeyFrame) ------------------------------------------------------
def _rot_from_rotvec(r):
    th = np.linalg.norm(r)
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
    if th < 1e-9:
        return np.eye(3) + K
    return np.eye(3) + K * np.sin(th) / th + K @ K * (1 - np.cos(th)) / th ** 2


# EuRoC-like IMU: body -> camera-0 extrinsics, noise densities at 200 Hz (Examples/Stereo-Inertial/EuRoC.yaml)
EUROC_TBC = np.array([[0.0148655429818, -0.999880929698, 0.00414029679422, -0.0216401454975],
                      [0.999557249008, 0.0149672133247, 0.025715529948, -0.064676986768],
                      [-0.0257744366974, 0.00375618835797, 0.999660727178, 0.00981073058949],
                      [0, 0, 0, 1]])
IMU_FREQ = 200.0
IMU_NOISE = dict(ng=1.7e-4, na=2.0e-3, ngw=1.9393e-05, naw=3.0e-3)


def imu_calib_diagonals(freq=IMU_FREQ, noise=IMU_NOISE):
    """Diagonals of IMU::Calib::Cov / CovWalk the way Tracking builds them (Tracking.cc ParseIMUParamFile:
    Calib(Tbc, Ng * sqrt(freq), Na * sqrt(freq), Ngw / sqrt(freq), Naw / sqrt(freq)); ImuTypes.cc:375-388)."""
    sf = np.sqrt(freq)
    ng, na, ngw, naw = noise["ng"] * sf, noise["na"] * sf, noise["ngw"] / sf, noise["naw"] / sf
    return (np.array([ng * ng] * 3 + [na * na] * 3, np.float32), np.array([ngw * ngw] * 3 + [naw * naw] * 3, np.float32))


def make_inertial_sequence(n=500, seed=0, n_imu=20, **kw):
    """Keyframe -> frame A -> frame B: (pA, pB).  pA is a PoseInertialOptimizationLastKeyFrame input; pB a
    PoseInertialOptimizationLastFrame input whose IMU samples continue the same motion: accF / gyroF / dtF since frame A
    (mpImuPreintegratedFrame) and acc / gyro / dt since the keyframe (mpImuPreintegrated).  The previous-frame state and
    prior of pB are frame A's optimisation results (not part of the dict)."""
    pA = make_inertial_problem(n, seed, n_imu, **kw)
    pB = make_inertial_problem(n, seed, 2 * n_imu, _obs_seed=1, **kw)
    assert np.array_equal(pA["acc"], pB["acc"][:n_imu])      # same motion and noise stream
    pB["accF"], pB["gyroF"], pB["dtF"] = pB["acc"][n_imu:], pB["gyro"][n_imu:], pB["dt"][n_imu:]
    return pA, pB


def tumvi_rig28():
    """Fisheye rig as the inertial entry points take it: left KB8 (8), right KB8 (8), Trl rotation (9, row-major) +
    translation (3)."""
    Trl = np.linalg.inv(TUMVI_T_C1_C2)
    return np.concatenate([TUMVI_CAM_L, TUMVI_CAM_R, Trl[:3, :3].ravel(), Trl[:3, 3]]).astype(np.float32)


def make_inertial_problem(n=500, seed=0, n_imu=20, outlier_frac=0.1, mono_frac=0.3, rot_deg=1.0, trans=0.03, cam=EUROC_CAM,
                          _obs_seed=0, rig=False):
    """One PoseInertialOptimizationLastKeyFrame input: the last keyframe's state, n_imu IMU samples of a smooth motion
    (constant body angular rate, constant world acceleration) between keyframe and frame, map points seen from the
    frame's true pose, and a perturbed initial frame state.  States: Rwb (9), twb, v, bg, ba."""
    rng = np.random.default_rng(0x1A70 + seed)
    g = np.array([0, 0, -9.81])
    R1 = _rot_from_rotvec(rng.normal(0, 0.3, 3)); p1 = rng.normal(0, 0.5, 3); v1 = rng.normal(0, 0.8, 3)
    bg = rng.normal(0, 0.01, 3); ba = rng.normal(0, 0.05, 3)
    w_b = rng.normal(0, 0.4, 3); a_w = rng.normal(0, 1.0, 3)
    dt = 1.0 / IMU_FREQ
    acc, gyro, dts = [], [], []
    for i in range(n_imu):
        tm = (i + 0.5) * dt
        Rm = R1 @ _rot_from_rotvec(w_b * tm)
        acc.append(Rm.T @ (a_w - g) + ba + rng.normal(0, 0.02, 3))
        gyro.append(w_b + bg + rng.normal(0, 0.002, 3))
        dts.append(dt)
    T = n_imu * dt
    rng = np.random.default_rng([0x1A71 + seed, _obs_seed, n_imu])   # map points / observations / initial guess
    R2 = R1 @ _rot_from_rotvec(w_b * T); v2 = v1 + a_w * T; p2 = p1 + v1 * T + 0.5 * a_w * T * T
    Tbc = EUROC_TBC
    Rcb = Tbc[:3, :3].T; tcb = -Rcb @ Tbc[:3, 3]
    Rcw = Rcb @ R2.T; tcw = Rcb @ (-R2.T @ p2) + tcb
    Xc = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(1.5, 25, n)], 1)
    Xw = (Xc - tcw) @ Rcw          # Rcw^T (Xc - tcw)
    z = Xc[:, 2]
    octave = rng.integers(0, 8, n); sigma = 1.2 ** octave
    n_left = n
    if rig:   # fisheye rig: features [0, n_left) seen by the left KB8 camera, the rest by the right one; all monocular
        n_left = int(0.55 * n)
        Trl = np.linalg.inv(TUMVI_T_C1_C2)
        uv = np.zeros((n, 2))
        uv[:n_left] = kb8_project(TUMVI_CAM_L, Xc[:n_left])
        uv[n_left:] = kb8_project(TUMVI_CAM_R, Xc[n_left:] @ Trl[:3, :3].T + Trl[:3, 3])
        u, v, ur = uv[:, 0], uv[:, 1], np.full(n, -1.0)
        sigma = sigma * 0.5
    else:
        u = cam["fx"] * Xc[:, 0] / z + cam["cx"]; v = cam["fy"] * Xc[:, 1] / z + cam["cy"]; ur = u - cam["bf"] / z
    u = u + rng.normal(0, 1, n) * sigma; v = v + rng.normal(0, 1, n) * sigma; ur = ur + rng.normal(0, 1, n) * sigma
    out = rng.random(n) < outlier_frac
    u[out] += rng.choice([-1, 1], out.sum()) * rng.uniform(15, 40, out.sum())
    v[out] += rng.choice([-1, 1], out.sum()) * rng.uniform(15, 40, out.sum())
    mono = (rng.random(n) < mono_frac) | rig
    ur[mono] = -1
    has = (rng.random(n) < 0.9).astype(np.uint8)
    R0 = R2 @ _rot_from_rotvec(rng.normal(0, 1, 3) / np.sqrt(3) * np.deg2rad(rot_deg))
    state0 = np.concatenate([R0.ravel(), p2 + rng.normal(0, trans, 3), v2 + rng.normal(0, 0.05, 3), bg, ba]).astype(np.float32)
    kf = np.concatenate([R1.ravel(), p1, v1, bg, ba]).astype(np.float32)
    return dict(hasMP=has, obs=np.stack([u, v, ur], 1).astype(np.float32), invSigma2=(1.0 / sigma ** 2).astype(np.float32),
                Xw=Xw.astype(np.float32), close=(z < 10).astype(np.uint8), state0=state0, kfState=kf,
                acc=np.array(acc, np.float32), gyro=np.array(gyro, np.float32), dt=np.array(dts, np.float32),
                bias=np.concatenate([ba, bg]).astype(np.float32),      # IMU::Bias order: acc then gyro
                Tbc12=np.concatenate([Tbc[:3, :3].ravel(), Tbc[:3, 3]]).astype(np.float32), cam=cam,
                true=np.concatenate([R2.ravel(), p2, v2, bg, ba]), outlier_truth=out, Nleft=n_left,
                rig28=tumvi_rig28() if rig else None)


def make_inertial_ba_problem(n_opt=10, n_fixed_vis=6, n_points=1500, n_imu=40, seed=0, outlier_frac=0.03, mono_frac=0.25,
                             cam=EUROC_CAM, rig=False):
    """LocalInertialBA input: a temporal chain keyframe 0 (fixed, with IMU state) -> n_opt optimizable keyframes, plus
    n_fixed_vis fixed keyframes that only observe points.  Each link carries n_imu IMU samples of a smooth motion
    (per-link constant body rate and world acceleration).  States: Rwb (9), twb, v, bg, ba; kfKind 0 / 1 / 2 as in
    morb_local_inertial_ba."""
    rng = np.random.default_rng(0x1BA0 + seed)
    g = np.array([0, 0, -9.81])
    dt = 1.0 / IMU_FREQ
    bg = rng.normal(0, 0.01, 3); ba = rng.normal(0, 0.05, 3)
    Tbc = EUROC_TBC
    Rcb = Tbc[:3, :3].T; tcb = -Rcb @ Tbc[:3, 3]
    # the camera looks along +z of the camera frame: start with the body oriented so that the camera faces world +x
    R = _rot_from_rotvec(rng.normal(0, 0.1, 3)); p = rng.normal(0, 0.2, 3); v = np.array([0.6, 0.1, 0.0]) + rng.normal(0, 0.1, 3)
    states = [(R, p, v)]
    acc, gyro, dts, start = [], [], [], [0]
    for k in range(n_opt):
        w_b = rng.normal(0, 0.15, 3); a_w = rng.normal(0, 0.5, 3)
        for i in range(n_imu):
            tm = (i + 0.5) * dt
            Rm = R @ _rot_from_rotvec(w_b * tm)
            acc.append(Rm.T @ (a_w - g) + ba + rng.normal(0, 0.02, 3))
            gyro.append(w_b + bg + rng.normal(0, 0.002, 3))
            dts.append(dt)
        T = n_imu * dt
        R, p, v = R @ _rot_from_rotvec(w_b * T), p + v * T + 0.5 * a_w * T * T, v + a_w * T
        states.append((R, p, v))
        start.append(len(dts))
    # visual-only fixed keyframes: near the start of the chain, slightly displaced
    for k in range(n_fixed_vis):
        R0, p0, _ = states[rng.integers(0, min(3, len(states)))]   # (a one-keyframe window has two states)
        states.append((R0 @ _rot_from_rotvec(rng.normal(0, 0.05, 3)), p0 + rng.normal(0, 0.15, 3), np.zeros(3)))
    nKF = len(states)
    kind = np.array([1] + [0] * n_opt + [2] * n_fixed_vis, np.uint8)
    cams = [(Rcb @ Rk.T, Rcb @ (-Rk.T @ pk) + tcb) for Rk, pk, _ in states]
    # points in front of the middle keyframe's camera
    Rm, tm_ = cams[n_opt // 2]
    Xc = np.stack([rng.uniform(-4, 4, n_points), rng.uniform(-2.5, 2.5, n_points), rng.uniform(2, 20, n_points)], 1)
    X = (Xc - tm_) @ Rm
    eKF, eMP, eObs, eInv, eRight = [], [], [], [], []
    Trl = np.linalg.inv(TUMVI_T_C1_C2)
    depth_ref = np.full(n_points, 1e9)
    for j in range(n_points):
        ks = rng.choice(nKF, size=min(int(rng.integers(3, 9)), nKF), replace=False)
        for k in ks:
            Rcw, tcw = cams[k]
            xc = Rcw @ X[j] + tcw
            if xc[2] < 0.5:
                continue
            octv = int(rng.integers(0, 8)); s = 1.2 ** octv
            right = 0
            if rig:   # one monocular observation on the left or on the right KB8 camera
                right = int(rng.random() < 0.45)
                xr = Trl[:3, :3] @ xc + Trl[:3, 3] if right else xc
                if xr[2] < 0.5:
                    continue
                u, vv = kb8_project(TUMVI_CAM_R if right else TUMVI_CAM_L, xr[None])[0]
                if not (0 <= u < 512 and 0 <= vv < 512):
                    continue
                s *= 0.5
                o = np.array([u, vv, -1.0]) + np.array([rng.normal(0, 1) * s, rng.normal(0, 1) * s, 0.0])
            else:
                u = cam["fx"] * xc[0] / xc[2] + cam["cx"]; vv = cam["fy"] * xc[1] / xc[2] + cam["cy"]
                if not (0 <= u < 752 and 0 <= vv < 480):
                    continue
                o = np.array([u, vv, u - cam["bf"] / xc[2]]) + rng.normal(0, 1, 3) * s
            if rng.random() < outlier_frac:
                o[:2] += rng.choice([-1, 1], 2) * rng.uniform(15, 30, 2)
            if not rig and rng.random() < mono_frac:
                o[2] = -1
            eKF.append(k); eMP.append(j); eObs.append(o); eInv.append(1.0 / (s * s)); eRight.append(right)
            depth_ref[j] = min(depth_ref[j], xc[2])
    true = np.stack([np.concatenate([Rk.ravel(), pk, vk, bg, ba]) for Rk, pk, vk in states])
    init = true.copy()
    for k in range(nKF):
        if kind[k] == 0:
            Rk = states[k][0] @ _rot_from_rotvec(rng.normal(0, 1, 3) / np.sqrt(3) * np.deg2rad(0.5))
            init[k, :9] = Rk.ravel(); init[k, 9:12] += rng.normal(0, 0.02, 3); init[k, 12:15] += rng.normal(0, 0.03, 3)
            init[k, 15:18] += rng.normal(0, 0.001, 3); init[k, 18:21] += rng.normal(0, 0.005, 3)
    iKF1 = np.arange(0, n_opt, dtype=np.int32); iKF2 = np.arange(1, n_opt + 1, dtype=np.int32)
    return dict(kfState=init.astype(np.float32), kfKind=kind, mpPos=(X + rng.normal(0, 0.03, X.shape)).astype(np.float32),
                mpClose=(depth_ref < 10).astype(np.uint8), eKF=np.array(eKF, np.int32), eMP=np.array(eMP, np.int32),
                eObs=np.array(eObs, np.float32), eInvSigma2=np.array(eInv, np.float32), iKF1=iKF1, iKF2=iKF2,
                iRobust=(iKF1 == 0).astype(np.uint8), iInfoScale=np.where(iKF1 == 0, 1e-2, 1.0).astype(np.float32),
                imuStart=np.array(start, np.int32), acc=np.array(acc, np.float32), gyro=np.array(gyro, np.float32),
                dt=np.array(dts, np.float32), bias=np.concatenate([ba, bg]).astype(np.float32),
                Tbc12=np.concatenate([Tbc[:3, :3].ravel(), Tbc[:3, 3]]).astype(np.float32), cam=cam, true=true, truePts=X,
                eRight=np.array(eRight, np.uint8), rig28=tumvi_rig28() if rig else None)


# ---- Optimizer::InertialOptimization (IMU initialisation: velocities, biases, gravity direction, scale) ----------------------
def make_inertial_optimization_problem(n_kf=20, seed=0, mono=True, s_true=1.0, n_imu=40, imu_freq=IMU_FREQ, noise=True, fixed_vel=False,
                                       prior_g=1e2, prior_a=1e10, broken=(), outlier_links=(), gyro_bias_offset=None, bias_sigma=(0.01, 0.05),
                                       rwg_deg=25.0):
    """One InertialOptimization input: n_kf keyframes, n_imu IMU samples apart, on a smooth trajectory with acceleration and rotation
    excitation (sinusoidal position, integrated sinusoidal body rate).  The IMU samples (imu_freq, known biases, noise from IMU_NOISE when
    `noise`) were integrated with the bias `bias` (zero, as LocalMapping::InitializeIMU has it); the world frame is rotated off gravity by a
    random Rwg_true of about rwg_deg degrees; positions (and so velocities) are divided by s_true, the monocular map's unknown scale.
    Initial velocities by finite differences and the initial Rwg from the summed delta-velocities, as LocalMapping.cc:1165-1193 prepares
    them.  broken: keyframes whose link to their predecessor is missing; outlier_links: keyframes whose link's samples are grossly wrong;
    gyro_bias_offset: the norm (rad/s) of the true gyro bias instead of a random one.
    Keys: kfState [n, 21] f32 (Rwb, twb, velocity, gyro bias, acc bias), hasLink [n] u8, imuStart [n + 1] i32 with acc / gyro / dt (keyframe k
    owns the samples since keyframe k - 1; keyframe 0 owns one unused sample), bias [6] f32 (IMU::Bias order: acc, gyro), flags (bit 0 bMono,
    bit 1 bFixedVel), prior2 f32 [2], global16 f64 [16] (Rwg, scale, bg, ba), and the truth: Rwg_true, s_true, bg_true, ba_true, v_true."""
    rng = np.random.default_rng([0x10A7, seed, n_kf])
    dt = 1.0 / imu_freq
    G = 9.81
    Rwg_true = _rot_from_rotvec(rng.normal(0, 1, 3) / np.sqrt(3) * np.deg2rad(rwg_deg))
    g_w = Rwg_true @ np.array([0, 0, -G])
    bg_t = rng.normal(0, bias_sigma[0], 3); ba_t = rng.normal(0, bias_sigma[1], 3)
    if gyro_bias_offset is not None:
        d = rng.normal(0, 1, 3)
        bg_t = d / np.linalg.norm(d) * gyro_bias_offset
    amp = rng.uniform(0.3, 0.8, 3); om = rng.uniform(1.5, 3.5, 3); ph = rng.uniform(0, 2 * np.pi, 3)
    wamp = rng.uniform(0.2, 0.6, 3); wom = rng.uniform(1.0, 3.0, 3); wph = rng.uniform(0, 2 * np.pi, 3)
    pos = lambda t: amp * np.sin(om * t + ph)
    vel = lambda t: amp * om * np.cos(om * t + ph)
    accw = lambda t: -amp * om * om * np.sin(om * t + ph)
    wb = lambda t: wamp * np.sin(wom * t + wph)
    ng, na = (noise_v * np.sqrt(imu_freq) for noise_v in (IMU_NOISE["ng"], IMU_NOISE["na"]))
    R = _rot_from_rotvec(rng.normal(0, 0.3, 3))
    Rs, ps, vs = [R], [pos(0.0)], [vel(0.0)]
    acc, gyro, dts, start = [np.zeros(3)], [np.zeros(3)], [dt], [0, 1]
    for k in range(1, n_kf):
        for i in range(n_imu):
            tm = ((k - 1) * n_imu + i + 0.5) * dt
            w = wb(tm)
            Rm = R @ _rot_from_rotvec(w * dt / 2)
            a = Rm.T @ (accw(tm) - g_w) + ba_t
            gy = w + bg_t
            if noise:
                a = a + rng.normal(0, na, 3); gy = gy + rng.normal(0, ng, 3)
            if k in outlier_links:
                a = a + np.array([3.0, -2.0, 2.5])
            acc.append(a); gyro.append(gy); dts.append(dt)
            R = R @ _rot_from_rotvec(w * dt)
        tk = k * n_imu * dt
        Rs.append(R); ps.append(pos(tk)); vs.append(vel(tk))
        start.append(len(dts))
    P = np.array(ps) / s_true
    V = np.zeros((n_kf, 3))
    has = np.ones(n_kf, np.uint8); has[0] = 0
    for k in broken:
        has[k] = 0
    acc, gyro, dts = np.array(acc, np.float32), np.array(gyro, np.float32), np.array(dts, np.float32)
    # LocalMapping.cc:1165-1193: dirG -= Rwb(prev) * dV, velocities by finite differences; dV of the zero-bias integration
    dirG = np.zeros(3)
    for k in range(1, n_kf):
        if not has[k]:
            continue
        dR, dV = np.eye(3), np.zeros(3)
        for i in range(start[k], start[k + 1]):
            dV = dV + dR @ acc[i].astype(np.float64) * dts[i]
            dR = dR @ _rot_from_rotvec(gyro[i].astype(np.float64) * dts[i])
        dirG -= Rs[k - 1] @ dV
        T = float(dts[start[k]:start[k + 1]].sum())
        V[k] = (P[k] - P[k - 1]) / T
        V[k - 1] = V[k]
    dirG = dirG / np.linalg.norm(dirG)
    gI = np.array([0, 0, -1.0])
    vx = np.cross(gI, dirG)
    Rwg0 = _rot_from_rotvec(vx * np.arccos(np.clip(gI @ dirG, -1, 1)) / max(np.linalg.norm(vx), 1e-12))
    st = np.zeros((n_kf, 21), np.float32)
    for k in range(n_kf):
        st[k, :9] = Rs[k].ravel(); st[k, 9:12] = P[k]; st[k, 12:15] = V[k]
    g16 = np.concatenate([Rwg0.ravel(), [1.0], np.zeros(3), np.zeros(3)])
    return dict(kfState=st, hasLink=has, imuStart=np.array(start, np.int32), acc=acc, gyro=gyro, dt=dts, bias=np.zeros(6, np.float32),
                flags=(1 if mono else 0) | (2 if fixed_vel else 0), prior2=np.array([prior_g, prior_a], np.float32), global16=g16,
                Rwg_true=Rwg_true, s_true=float(s_true), bg_true=bg_t, ba_true=ba_t, v_true=np.array(vs) / s_true)


def pack_inertial_optimization_problems(probs, pres, device, pad_rows=0):
    """Problems of make_inertial_optimization_problem with their preintegrations (pres[p]: [n_p, 310] f32, or one device tensor of all rows)
    as the device tensors of Optimizer.InertialOptimization: (kfStart, kfState, hasLink, pre, flags, prior2, global16); pad_rows extra
    keyframe rows (filled with a pattern) follow the last problem."""
    import torch
    ns = [p["kfState"].shape[0] for p in probs]
    start = np.cumsum([0] + ns).astype(np.int32)
    st = np.concatenate([p["kfState"] for p in probs] + [np.full((pad_rows, 21), 7.25, np.float32)])
    hl = np.concatenate([p["hasLink"] for p in probs] + [np.ones(pad_rows, np.uint8)])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if isinstance(pres, (list, tuple)):
        pre = t(np.concatenate(list(pres) + [np.zeros((pad_rows, pres[0].shape[1]), np.float32)]).astype(np.float32))
    else:
        pre = pres
    return (t(start), t(st), t(hl), pre, t(np.array([p["flags"] for p in probs], np.int32)),
            t(np.stack([p["prior2"] for p in probs]).astype(np.float32)), t(np.stack([p["global16"] for p in probs]).astype(np.float64)))


# ---- Optimizer::OptimizeSim3 (two keyframes of one scene under a known Sim3) -----------------------------------
SIM3_PINHOLE9 = np.array([0, EUROC_CAM["fx"], EUROC_CAM["fy"], EUROC_CAM["cx"], EUROC_CAM["cy"], 0, 0, 0, 0], np.float32)


def sim3_camera9(kind):
    """morb_optimize_sim3_batch camera record: kind (0 pinhole, 1 KannalaBrandt8) + 8 parameters."""
    if kind == "pinhole":
        return SIM3_PINHOLE9.copy()
    return np.concatenate([[1.0], TUMVI_CAM_L]).astype(np.float32)


def _sim3_project(kind, X):
    c = sim3_camera9(kind)[1:].astype(np.float64)
    if kind == "pinhole":
        return np.stack([c[0] * X[:, 0] / X[:, 2] + c[2], c[1] * X[:, 1] / X[:, 2] + c[3]], 1)
    return kb8_project(c, X)


def make_sim3_problem(n=400, seed=0, cam1="pinhole", cam2="pinhole", fix_scale=False, outlier_frac=0.0, neg_i2_frac=0.0, bad_frac=0.0,
                      no_mp1_frac=0.0, unmatched_frac=0.1, perturb=True, noise_px=0.0, th2=10.0):
    """One OptimizeSim3 input: n KF1 features, most matched to a KF2 map point; x1 = S12 * x2 with a known S12 (scale != 1 unless
    fix_scale, the stereo case).  Options: KB8 or pinhole on either side, gross outliers (obs1 moved 20 - 60 px), matches whose map point
    is not seen in KF2 (i2 = -1), bad map points, matches without pMP1, a perturbed initial S12 (perturb) and pixel noise.
    Returns a dict of the morb_optimize_sim3_batch per-problem arrays plus the true S12 and the planted outliers."""
    rng = np.random.default_rng(0x53B3 + seed)
    lev = (1.2 ** np.arange(8)) ** 2
    inv_level = (1.0 / lev).astype(np.float32)
    # scene in KF1's camera frame, inside both fields of view
    z1 = rng.uniform(2.0, 8.0, n)
    half = 0.55 if cam1 == "pinhole" else 1.2
    X1c = np.stack([rng.uniform(-half, half, n) * z1, rng.uniform(-0.4, 0.4, n) * z1, z1], 1)
    s = 1.0 if fix_scale else float(rng.uniform(0.6, 1.6))
    q = _quat_from_rotvec(rng.normal(0, 0.08, 3))
    t = rng.normal(0, 0.15, 3)
    S12 = np.concatenate([q, t, [s]])                      # x1 = s R x2 + t
    qc = q * np.array([-1, -1, -1, 1.0])
    X2c = np.array([_quat_rot(qc, (x - t) / s) for x in X1c])
    # keyframe poses (world -> camera) and world positions of the two map points of each match
    def pose():
        return _rot_from_rotvec(rng.normal(0, 0.3, 3)), rng.normal(0, 1.0, 3)
    R1, t1 = pose()
    R2, t2 = pose()
    Xw1 = ((X1c - t1) @ R1).astype(np.float32)
    Xw2 = ((X2c - t2) @ R2).astype(np.float32)
    T1w = np.concatenate([R1.reshape(-1), t1]).astype(np.float32)
    T2w = np.concatenate([R2.reshape(-1), t2]).astype(np.float32)
    obs1 = _sim3_project(cam1, X1c) + rng.normal(0, noise_px, (n, 2))
    obs2 = _sim3_project(cam2, X2c) + rng.normal(0, noise_px, (n, 2))
    oct1 = rng.integers(0, 8, n)
    oct2 = rng.integers(0, 8, n)
    outlier = rng.random(n) < outlier_frac
    shift = rng.uniform(20, 60, (n, 2)) * rng.choice([-1, 1], (n, 2))
    obs1[outlier] += shift[outlier]
    matched = rng.random(n) >= unmatched_frac
    has_mp1 = rng.random(n) >= no_mp1_frac
    bad1 = rng.random(n) < bad_frac / 2
    bad2 = rng.random(n) < bad_frac / 2
    entry = (matched.astype(np.uint8) | (has_mp1.astype(np.uint8) << 1) | (bad1.astype(np.uint8) << 2) |
             (bad2.astype(np.uint8) << 3)).astype(np.uint8)
    i2 = rng.permutation(4 * n)[:n].astype(np.int32)
    i2[rng.random(n) < neg_i2_frac] = -1
    inv2 = inv_level[oct2]
    inv2[i2 < 0] = inv_level[0]        # the reference's stand-in keypoint of an i2 < 0 match keeps octave 0
    S0 = S12.copy()
    if perturb:
        S0[:4] = _quat_mul(_quat_from_rotvec(rng.normal(0, 0.01, 3)), q)
        S0[4:7] = t + rng.normal(0, 0.02, 3)
        S0[7] = s * (1.0 if fix_scale else float(np.exp(rng.normal(0, 0.03))))
    return dict(n=n, entry=entry, Xw1=Xw1, Xw2=Xw2, i2=i2, obs1=obs1.astype(np.float32), inv1=inv_level[oct1],
                obs2=obs2.astype(np.float32), inv2=inv2, T1w=T1w, T2w=T2w, cam1=sim3_camera9(cam1), cam2=sim3_camera9(cam2),
                th2=np.float32(th2), fix_scale=bool(fix_scale), S12=S0.astype(np.float64), S12_true=S12, outlier=outlier & matched)


def pack_sim3_problems(probs, device):
    """make_sim3_problem dicts -> the padded [P, cap] torch tensors of Optimizer.OptimizeSim3 on `device` (cap = the largest n)."""
    import torch
    P, cap = len(probs), max(max(p["n"] for p in probs), 1)

    def stack(key, shape, dtype):
        a = np.zeros((P, cap) + shape, dtype)
        for k, p in enumerate(probs):
            a[k, :p["n"]] = p[key]
        return torch.from_numpy(a).to(device)
    t = {"entry": stack("entry", (), np.uint8), "Xw1": stack("Xw1", (3,), np.float32), "Xw2": stack("Xw2", (3,), np.float32),
         "i2": stack("i2", (), np.int32), "obs1": stack("obs1", (2,), np.float32), "obs2": stack("obs2", (2,), np.float32),
         "inv1": stack("inv1", (), np.float32), "inv2": stack("inv2", (), np.float32)}
    for k in ("T1w", "T2w", "cam1", "cam2"):
        t[k] = torch.from_numpy(np.stack([p[k] for p in probs]).astype(np.float32)).to(device)
    t["th2"] = torch.tensor([float(p["th2"]) for p in probs], dtype=torch.float32, device=device)
    t["fix"] = torch.tensor([int(p["fix_scale"]) for p in probs], dtype=torch.uint8, device=device)
    t["S12"] = torch.from_numpy(np.stack([p["S12"] for p in probs]).astype(np.float64)).to(device)
    t["count"] = torch.tensor([p["n"] for p in probs], dtype=torch.int32, device=device)
    return t


def make_sim3_solver_problem(n=400, seed=0, cam1="pinhole", cam2="pinhole", fix_scale=False, outlier_frac=0.3, bad_frac=0.04,
                             no_mp1_frac=0.03, unmatched_frac=0.1, neg_idx_frac=0.03, dup_frac=0.02, collinear=False, identical=False,
                             noise_px=0.3,
                             min_inliers=20, probability=0.99, max_iterations=300):
    """One Sim3Solver input on make_sim3_problem's geometry: n KF1 features; entry bits 0-3 as there, bit 4 / 5 = a negative keyframe
    index of pMP1 / pMP2; outliers move pMP2's world position by ~0.5 m (the solver projects map points, not keypoints); octaves
    give sigma2 = 1.44^octave on each side (pKFm's octave for side 2); dup_frac of the features repeat another feature's points;
    collinear puts every pMP1 / pMP2 pair on one line, identical every pair on one point (every triple is degenerate).  Returns a dict of the morb_sim3_solver_batch
    per-problem arrays and parameters."""
    if n == 0:
        p = make_sim3_solver_problem(1, seed, cam1, cam2, fix_scale, min_inliers=min_inliers, probability=probability,
                                     max_iterations=max_iterations)
        for k in ("entry", "Xw1", "Xw2", "sigma2_1", "sigma2_2", "outlier"):
            p[k] = p[k][:0]
        p["n"] = 0
        return p
    base = make_sim3_problem(n=n, seed=seed, cam1=cam1, cam2=cam2, fix_scale=fix_scale, outlier_frac=0.0, bad_frac=bad_frac,
                             no_mp1_frac=no_mp1_frac, unmatched_frac=unmatched_frac, perturb=False, noise_px=0.0)
    rng = np.random.default_rng(0x5A3C + seed)
    Xw1, Xw2 = base["Xw1"].astype(np.float64), base["Xw2"].astype(np.float64)
    Xw2 = Xw2 + rng.normal(0, noise_px * 2e-3, Xw2.shape)       # ~noise_px pixels at a few metres
    outlier = rng.random(n) < outlier_frac
    Xw2[outlier] += rng.normal(0, 0.5, (int(outlier.sum()), 3))
    if n > 1:
        dup = np.nonzero(rng.random(n) < dup_frac)[0]
        src = rng.integers(0, n, len(dup))
        Xw1[dup], Xw2[dup] = Xw1[src], Xw2[src]
    if collinear:
        u = rng.uniform(-1, 1, n)[:, None]
        Xw1 = Xw1[0] + u * np.array([0.3, 0.1, 0.05])
        Xw2 = Xw2[0] + u * np.array([0.2, -0.1, 0.04])
    if identical:
        Xw1, Xw2 = np.repeat(Xw1[:1], n, 0), np.repeat(Xw2[:1], n, 0)
    entry = base["entry"].copy()
    entry |= ((rng.random(n) < neg_idx_frac / 2).astype(np.uint8) << 4)
    entry |= ((rng.random(n) < neg_idx_frac / 2).astype(np.uint8) << 5)
    lev = (1.2 ** np.arange(8)) ** 2
    oct1, oct2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    return dict(n=n, entry=entry.astype(np.uint8), Xw1=Xw1.astype(np.float32), Xw2=Xw2.astype(np.float32),
                sigma2_1=lev[oct1].astype(np.float32), sigma2_2=lev[oct2].astype(np.float32), T1w=base["T1w"], T2w=base["T2w"],
                cam1=base["cam1"], cam2=base["cam2"], fix_scale=bool(fix_scale), min_inliers=int(min_inliers),
                probability=float(probability), max_iterations=int(max_iterations), outlier=outlier, S12_true=base["S12_true"])


def libc_rand(seed, count):
    """count values of the C library's rand() after srand(seed): the draws DUtils::Random::RandomInt makes in the reference."""
    import ctypes
    import ctypes.util
    libc = ctypes.CDLL(ctypes.util.find_library("c"))
    libc.srand(ctypes.c_uint(seed))
    return np.array([libc.rand() for _ in range(count)], np.int32)


def pack_sim3_solver_problems(probs, device, rand=None, cap=None):
    """make_sim3_solver_problem dicts -> the torch tensors of Optimizer.Sim3Solver on `device` (cap = the largest n unless given):
    params u8 [P, 192], entry, Xw1, Xw2, sigma2_1, sigma2_2, rand i32 [P, randCap] (the given list of arrays, zero padded) and a zeroed
    state u8 [P, 212]."""
    import torch
    from .optimizer import SIM3_SOLVER_PARAMS, SIM3_SOLVER_STATE
    P = len(probs)
    cap = cap or max(max(p["n"] for p in probs), 1)

    def stack(key, shape, dtype):
        a = np.zeros((P, cap) + shape, dtype)
        for k, p in enumerate(probs):
            a[k, :p["n"]] = p[key]
        return torch.from_numpy(a).to(device)
    prm = np.zeros(P, SIM3_SOLVER_PARAMS)
    for k, p in enumerate(probs):
        prm[k]["T1w"], prm[k]["T2w"], prm[k]["cam1"], prm[k]["cam2"] = p["T1w"], p["T2w"], p["cam1"], p["cam2"]
        prm[k]["probability"], prm[k]["minInliers"], prm[k]["maxIterations"] = p["probability"], p["min_inliers"], p["max_iterations"]
        prm[k]["fixScale"], prm[k]["n"] = int(p["fix_scale"]), p["n"]
    t = {"entry": stack("entry", (), np.uint8), "Xw1": stack("Xw1", (3,), np.float32), "Xw2": stack("Xw2", (3,), np.float32),
         "sigma2_1": stack("sigma2_1", (), np.float32), "sigma2_2": stack("sigma2_2", (), np.float32)}
    t["params"] = torch.from_numpy(np.frombuffer(prm.tobytes(), np.uint8).reshape(P, -1).copy()).to(device)
    t["state"] = torch.zeros((P, SIM3_SOLVER_STATE.itemsize), dtype=torch.uint8, device=device)
    if rand is not None:
        rc = max(max(len(r) for r in rand), 1)
        a = np.zeros((P, rc), np.int32)
        for k, r in enumerate(rand):
            a[k, :len(r)] = r
        t["rand"] = torch.from_numpy(a).to(device)
    return t


# ---- MLPnPsolver (one frame against the map points of a relocalisation candidate) ------------------------------
def make_mlpnp_problem(n=100, seed=0, cam="pinhole", outlier_frac=0.3, noise_px=0.5, bad_frac=0.03, unmatched_frac=0.1, planar=False,
                       dup_frac=0.0, identical=False, beyond_frac=0.0, probability=0.99, min_inliers=10, max_iterations=300, min_set=6,
                       epsilon=0.5, th2=5.991):
    """One MLPnPsolver input: n features of a frame with a true pose Tcw; map points in front of the camera (on the world plane z = 0,
    exactly, when planar), octaves U{0..7} with sigma2 = 1.44^octave, pixel noise noise_px * 1.2^octave, gross outliers moved by
    +-20..80 px per axis.  entry bit 0 = matched, bit 1 = bad map point, bit 2 = a feature index beyond mvKeysUn (beyond_frac);
    dup_frac of the features repeat another feature's point and keypoint, identical makes all of them one.  The parameters default to
    Tracking::Relocalization's SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991).  Returns a dict of the morb_mlpnp_solver_batch
    per-problem arrays and parameters plus the true pose (Tcw_true, 4 x 4) and the planted outliers."""
    if n == 0:
        p = make_mlpnp_problem(1, seed, cam, probability=probability, min_inliers=min_inliers, max_iterations=max_iterations,
                               min_set=min_set, epsilon=epsilon, th2=th2)
        for k in ("entry", "uv", "sigma2", "Xw", "outlier"):
            p[k] = p[k][:0]
        p["n"] = 0
        return p
    rng = np.random.default_rng(0x3E77 + seed)
    R = _rot_from_rotvec(rng.normal(0, 0.35, 3))
    if planar:
        t = np.array([rng.normal(0, 0.3), rng.normal(0, 0.3), rng.uniform(3.5, 5.0)])
        Xw = np.stack([rng.uniform(-1.6, 1.6, n), rng.uniform(-1.2, 1.2, n), np.zeros(n)], 1)
    else:
        t = rng.normal(0, 0.8, 3)
        z = rng.uniform(2.0, 8.0, n)
        half = 0.55 if cam == "pinhole" else 1.2
        Xc = np.stack([rng.uniform(-half, half, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], 1)
        Xw = (Xc - t) @ R
    Xw = Xw.astype(np.float32)
    octave = rng.integers(0, 8, n)
    noise = rng.normal(0, 1.0, (n, 2)) * (noise_px * 1.2 ** octave)[:, None]
    outlier = rng.random(n) < outlier_frac
    shift = rng.uniform(20, 80, (n, 2)) * rng.choice([-1, 1], (n, 2))
    dup = np.nonzero(rng.random(n) < dup_frac)[0] if n > 1 else np.zeros(0, np.int64)
    src = rng.integers(0, n, len(dup))
    matched = rng.random(n) >= unmatched_frac
    bad = rng.random(n) < bad_frac
    beyond = rng.random(n) < beyond_frac
    uv = _sim3_project(cam, Xw.astype(np.float64) @ R.T + t) + noise
    uv[outlier] += shift[outlier]
    uv = uv.astype(np.float32)
    Xw[dup], uv[dup], octave[dup] = Xw[src], uv[src], octave[src]
    if identical:
        Xw, uv, octave = np.repeat(Xw[:1], n, 0), np.repeat(uv[:1], n, 0), np.repeat(octave[:1], n, 0)
    entry = (matched.astype(np.uint8) | (bad.astype(np.uint8) << 1) | (beyond.astype(np.uint8) << 2)).astype(np.uint8)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return dict(n=n, entry=entry, uv=uv, sigma2=(1.44 ** octave).astype(np.float32), Xw=Xw, cam=sim3_camera9(cam),
                probability=float(probability), min_inliers=int(min_inliers), max_iterations=int(max_iterations), min_set=int(min_set),
                epsilon=float(epsilon), th2=float(th2), Tcw_true=T, outlier=outlier)


def pack_mlpnp_problems(probs, device, rand=None, cap=None):
    """make_mlpnp_problem dicts -> the torch tensors of Optimizer.MLPnPsolver on `device` (cap = the largest n unless given): params u8
    [P, 72], entry, uv, sigma2, Xw, rand i32 [P, randCap] (the given list of arrays, zero padded), a zeroed state u8 [P, 168] and a
    zeroed bestInliers u8 [P, cap]."""
    import torch
    from .optimizer import MLPNP_SOLVER_PARAMS, MLPNP_SOLVER_STATE
    P = len(probs)
    cap = cap or max(max(p["n"] for p in probs), 1)

    def stack(key, shape, dtype):
        a = np.zeros((P, cap) + shape, dtype)
        for k, p in enumerate(probs):
            a[k, :p["n"]] = p[key]
        return torch.from_numpy(a).to(device)
    prm = np.zeros(P, MLPNP_SOLVER_PARAMS)
    for k, p in enumerate(probs):
        if not 6 <= p["min_set"] <= 16:
            raise ValueError("min_set outside [6, 16]")   # the entry point's argument error: the kernel cannot return one
        prm[k]["cam"], prm[k]["probability"], prm[k]["minInliers"] = p["cam"], p["probability"], p["min_inliers"]
        prm[k]["maxIterations"], prm[k]["minSet"], prm[k]["epsilon"], prm[k]["th2"], prm[k]["n"] = \
            p["max_iterations"], p["min_set"], p["epsilon"], p["th2"], p["n"]
    t = {"entry": stack("entry", (), np.uint8), "uv": stack("uv", (2,), np.float32), "sigma2": stack("sigma2", (), np.float32),
         "Xw": stack("Xw", (3,), np.float32)}
    t["params"] = torch.from_numpy(np.frombuffer(prm.tobytes(), np.uint8).reshape(P, -1).copy()).to(device)
    t["state"] = torch.zeros((P, MLPNP_SOLVER_STATE.itemsize), dtype=torch.uint8, device=device)
    t["bestInliers"] = torch.zeros((P, cap), dtype=torch.uint8, device=device)
    if rand is not None:
        rc = max(max(len(r) for r in rand), 1)
        a = np.zeros((P, rc), np.int32)
        for k, r in enumerate(rand):
            a[k, :len(r)] = r
        t["rand"] = torch.from_numpy(a).to(device)
    return t


# ---- TwoViewReconstruction (two frames of a monocular initialisation and vnMatches12) ---------------------------
TWO_VIEW_KINDS = ("general", "planar", "rotation", "outliers", "tiny", "small_baseline", "epipolar", "corners")


def make_two_view_problem(seed=0, kind="general", n1=300, n2=280, n_matches=200, noise_px=0.4, outlier_frac=None, sigma=1.0,
                          max_iterations=200, K4=(520.0, 522.0, 318.5, 241.0), width=640, height=480, corner_px=1.5):
    """One TwoViewReconstruction input: n1 / n2 undistorted keypoints of frames 1 and 2 (matched and unmatched ones in a seeded random
    order), vnMatches12 [n1] (frame-2 index or -1) with n_matches matches, a pinhole K4 = fx fy cx cy, and the ground truth T21 (4 x 4;
    the translation's length is not observable).  kind: "general" (points at depths 2.5 .. 9), "planar" (points on one tilted plane),
    "rotation" (a baseline of 1e-4: near-pure rotation), "outliers" (45 % of the matches wrong unless outlier_frac says otherwise),
    "tiny" (as general; meant for n_matches around 8), "small_baseline" (a clear winner whose parallax stays below one degree),
    "epipolar" (a fifth of the matches moved along their epipolar line to a negative depth: they pass CheckFundamental and fail
    CheckRT), "corners" (five corners of one tilted plane under a wide baseline, each matched n_matches / 5 times within corner_px
    pixels of the corner in frame 1: with corner_px = 0 the frame-1 positions of a corner's matches coincide, as one corner detected
    on several pyramid levels does; the one kind whose samples let SH exceed SF, see tests/two_view_corpus.py).  Matched keypoints carry
    Gaussian pixel noise noise_px in frame 2."""
    assert kind in TWO_VIEW_KINDS and n_matches <= min(n1, n2)
    rng = np.random.default_rng(0x7E01 + seed)
    fx, fy, cx, cy = K4
    if outlier_frac is None:
        outlier_frac = 0.45 if kind == "outliers" else 0.08
    R = _rot_from_rotvec(rng.normal(0, 0.06, 3))
    tdir = np.array([rng.choice([-1.0, 1.0]) * rng.uniform(0.7, 1.0), rng.normal(0, 0.25), rng.normal(0, 0.25)])
    tdir /= np.linalg.norm(tdir)
    base = {"rotation": 1e-4, "small_baseline": 0.08, "corners": rng.uniform(0.9, 1.3)}.get(kind, rng.uniform(0.35, 0.6))
    t = tdir * base
    m = n_matches
    u = np.stack([rng.uniform(30, width - 30, m), rng.uniform(30, height - 30, m)], 1)
    if kind == "corners":   # five corners of one plane, each detected many times within a pixel or two
        centre = np.stack([rng.uniform(60, width - 60, 5), rng.uniform(60, height - 60, 5)], 1)
        u = centre[np.arange(m) % 5] + rng.uniform(-corner_px, corner_px, (m, 2))
    ray = np.stack([(u[:, 0] - cx) / fx, (u[:, 1] - cy) / fy, np.ones(m)], 1)
    if kind in ("planar", "corners"):
        tilt = 0.6 if kind == "corners" else 0.25
        nrm = np.array([rng.normal(0, tilt), rng.normal(0, tilt), -1.0])
        nrm /= np.linalg.norm(nrm)
        z = 4.5 * nrm[2] / (ray @ nrm)   # the plane nrm . X = 4.5 nrm_z: depth 4.5 on the optical axis
    elif kind == "small_baseline":
        z = rng.uniform(5.5, 7.0, m)
    else:
        z = rng.uniform(2.5, 9.0, m)
    X1 = ray * z[:, None]
    X2 = X1 @ R.T + t
    v = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1)
    if kind == "epipolar":   # reflect the projection through the vanishing point of the ray: a negative depth on the same epipolar line
        Xinf = ray @ R.T
        vinf = np.stack([fx * Xinf[:, 0] / Xinf[:, 2] + cx, fy * Xinf[:, 1] / Xinf[:, 2] + cy], 1)
        moved = rng.random(m) < 0.2
        v[moved] = 2 * vinf[moved] - v[moved]
    v = v + rng.normal(0, noise_px, (m, 2))
    out = rng.random(m) < outlier_frac
    v[out] = np.stack([rng.uniform(0, width, int(out.sum())), rng.uniform(0, height, int(out.sum()))], 1)
    kp1 = np.stack([rng.uniform(0, width, n1), rng.uniform(0, height, n1)], 1)
    kp2 = np.stack([rng.uniform(0, width, n2), rng.uniform(0, height, n2)], 1)
    i1 = np.sort(rng.permutation(n1)[:m])
    i2 = rng.permutation(n2)[:m]
    kp1[i1], kp2[i2] = u, v
    matches = np.full(n1, -1, np.int32)
    matches[i1] = i2
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return dict(kind=kind, n1=n1, n2=n2, kp1=kp1.astype(np.float32), kp2=kp2.astype(np.float32), matches12=matches,
                K4=np.array(K4, np.float32), sigma=float(sigma), max_iterations=int(max_iterations), T21_true=T, outlier=out,
                noise_px=float(noise_px))


def pack_two_view_problems(probs, device, rand=None, cap=None):
    """make_two_view_problem dicts -> the torch tensors of Optimizer.TwoViewReconstruction on `device`: a keypoint pool kps u8 view of
    KP_DTYPE records [2 P, cap] (problem p owns images 2 p and 2 p + 1), img1 / img2 i32 [P], count i32 [2 P], matches12 i32 [P, cap]
    (-1 padded), K4 f32 [P, 4], sigma f32 [P], rand i32 [P, randCap] (the given list of arrays, zero padded).  cap = the largest frame
    unless given."""
    import torch
    from .capi import KP_DTYPE
    P = len(probs)
    cap = cap or max(max(max(p["n1"], p["n2"]) for p in probs), 1)
    kps = np.zeros((2 * P, cap), KP_DTYPE)
    count = np.zeros(2 * P, np.int32)
    m12 = np.full((P, cap), -1, np.int32)
    for k, p in enumerate(probs):
        for j, (key, n) in enumerate((("kp1", p["n1"]), ("kp2", p["n2"]))):
            kps[2 * k + j, :n]["x"], kps[2 * k + j, :n]["y"] = p[key][:, 0], p[key][:, 1]
            count[2 * k + j] = n
        m12[k, :p["n1"]] = p["matches12"]
    t = {"kps": torch.from_numpy(kps.view(np.uint8).reshape(2 * P, cap, KP_DTYPE.itemsize).copy()).to(device),
         "img1": torch.arange(0, 2 * P, 2, dtype=torch.int32).to(device), "img2": torch.arange(1, 2 * P, 2, dtype=torch.int32).to(device),
         "count": torch.from_numpy(count).to(device), "matches12": torch.from_numpy(m12).to(device),
         "K4": torch.from_numpy(np.stack([p["K4"] for p in probs]).astype(np.float32)).to(device),
         "sigma": torch.from_numpy(np.array([p["sigma"] for p in probs], np.float32)).to(device)}
    if rand is not None:
        rc = max(max(len(r) for r in rand), 1)
        a = np.zeros((P, rc), np.int32)
        for k, r in enumerate(rand):
            a[k, :len(r)] = r
        t["rand"] = torch.from_numpy(a).to(device)
    return t


def make_keyframe_database_scene(seed=0, nKF=70, nwords_voc=1000, words_per_kf=(20, 100), nmaps=2, cap=None, ncovis=10, nplaces=None,
                                 place_frac=0.85, place_words=None, dup_groups=0, dup_size=3, erased_frac=0.1, disjoint=2, bad_frac=0.08, bad_maps=(),
                                 nconn=4):
    """A keyframe database for KeyFrameDatabase::DetectNBestCandidates / DetectRelocalizationCandidates: nKF pool rows whose BoW
    vectors are L1-normalised TF-IDF-like doubles over a vocabulary of nwords_voc words, words ascending, as morb_bow_vector_batch
    leaves them.  The trajectory visits each of nplaces places twice (keyframe i is at place (2 i nplaces // nKF) % nplaces), the maps
    split it into nmaps consecutive parts; a place owns a pool of place_words (default hi) words, and a keyframe draws place_frac of its words_per_kf =
    (lo, hi) words from it and the rest from the whole vocabulary, so keyframes of one place share many words and all share a few.  Knobs: dup_groups groups of dup_size keyframes with IDENTICAL vectors (exact score ties), erased_frac of the
    rows outside the database (db_rank < 0), `disjoint` keyframes on words of their own that nobody else has (the top of the
    vocabulary is reserved for them), bad_frac bad keyframes, bad_maps = the maps that are bad.
    Returns a dict: word i32 [nKF, cap], value f64 [nKF, cap], count i32 [nKF], db_rank i32 [nKF] (a shuffled add order with holes),
    covis i32 [nKF, ncovis] (-1 padded, rows of every length from 0, neighbours by decreasing shared place), connected (a list of i32
    arrays: each keyframe's GetConnectedKeyFrames()), map_id i32 [nKF], flags u8 [nKF] (bit 0 bad, bit 1 the map is bad), and
    nwords_voc, nmaps, cap, ncovis."""
    rng = np.random.default_rng(seed)
    lo, hi = words_per_kf
    cap = cap or hi
    nplaces = nplaces or max(nKF // 16, 1)
    reserve = disjoint * hi
    common = nwords_voc - reserve
    assert common >= hi and cap >= hi
    idf = rng.uniform(0.5, 9.0, nwords_voc)
    place_pool = [rng.choice(common, size=min(common, place_words or hi), replace=False) for _ in range(nplaces)]
    word = np.zeros((nKF, cap), np.int32)
    value = np.zeros((nKF, cap), np.float64)
    count = np.zeros(nKF, np.int32)
    place = (np.arange(nKF) * 2 * nplaces // max(nKF, 1)) % nplaces     # every place is visited twice: loops, and merges across maps
    lonely = set(rng.choice(nKF, size=min(disjoint, nKF), replace=False).tolist())
    for i in range(nKF):
        n = int(rng.integers(lo, hi + 1))
        if i in lonely:
            k = sorted(lonely).index(i)
            w = common + k * hi + rng.choice(hi, size=n, replace=False)
        else:
            pool = place_pool[place[i]]
            n_place = min(int(round(place_frac * n)), len(pool))
            chosen = rng.choice(pool, size=n_place, replace=False)
            extra = rng.integers(0, common, 2 * (n - n_place) + 8)
            extra = extra[~np.isin(extra, chosen)]
            extra = extra[np.sort(np.unique(extra, return_index=True)[1])][:n - n_place]
            w = np.concatenate([chosen, extra]).astype(np.int64)
            n = len(w)
        w = np.sort(w)
        tf = rng.integers(1, 5, n).astype(np.float64)
        v = tf * idf[w]
        v = v / np.abs(v).sum()
        word[i, :n], value[i, :n], count[i] = w, v, n
    for g in range(dup_groups):     # identical vectors: the members of a group tie exactly, on any query
        members = [m for m in rng.choice(nKF, size=min(dup_size, nKF), replace=False).tolist() if m not in lonely]
        for m in members[1:]:
            word[m], value[m], count[m] = word[members[0]], value[members[0]], count[members[0]]
    in_db = np.ones(nKF, bool)
    in_db[rng.choice(nKF, size=min(int(np.ceil(erased_frac * nKF)), nKF), replace=False)] = False
    order = rng.permutation(nKF)
    db_rank = np.full(nKF, -1, np.int32)
    db_rank[order] = np.arange(nKF, dtype=np.int32)
    db_rank[~in_db] = -1
    map_id = (np.arange(nKF) * nmaps // max(nKF, 1)).astype(np.int32)
    flags = np.zeros(nKF, np.uint8)
    flags[rng.choice(nKF, size=min(int(np.ceil(bad_frac * nKF)), nKF), replace=False)] = 1
    for mp in bad_maps:
        flags[map_id == mp] |= 2
    covis = np.full((nKF, max(ncovis, 1)), -1, np.int32)[:, :ncovis]
    connected = []
    for i in range(nKF):
        near = [j for d in range(1, 2 * ncovis + nconn + 2) for j in (i - d, i + d) if 0 <= j < nKF]   # by index distance
        ncv = int(rng.integers(0, ncovis + 1)) if ncovis else 0
        pick = near[:max(2 * ncv, 1)]
        rng.shuffle(pick)
        if ncv and pick and rng.random() < 0.3:                       # now and then a far neighbour: the best keyframe of another map
            pick[0] = int(rng.integers(0, nKF))
            if pick[0] == i:
                pick[0] = (i + 1) % nKF
        row = list(dict.fromkeys(pick))[:ncv]
        covis[i, :len(row)] = row
        connected.append(np.array(sorted(set(near[:int(rng.integers(0, nconn + 1))])), np.int32))
    return dict(word=word, value=value, count=count, db_rank=db_rank, covis=np.ascontiguousarray(covis), connected=connected, map_id=map_id,
                flags=flags, nwords_voc=nwords_voc, nmaps=nmaps, cap=cap, ncovis=ncovis)


def keyframe_database_connected_csr(scene, queries):
    """The CSR (conn_start i32 [nq + 1], conn i32) of the connected sets of the query keyframes `queries` of a
    make_keyframe_database_scene dict, as morb_detect_n_best_candidates_batch reads them."""
    sets = [scene["connected"][int(q)] for q in queries]
    start = np.zeros(len(sets) + 1, np.int32)
    start[1:] = np.cumsum([len(s) for s in sets])
    conn = np.concatenate(sets).astype(np.int32) if sets and start[-1] else np.zeros(0, np.int32)
    return start, conn


# ---- LocalMapping::CreateNewMapPoints ---------------------------------------------------------------------------------------------------
NEW_MAP_POINT_KINDS = ("mono", "stereo1", "stereo2", "rig")
# what a match of the scene was built to be; the status it gets is the oracle's business
NEW_MAP_POINT_CATEGORIES = ("good", "low_parallax", "behind_both", "behind_2", "reproj1", "reproj2", "far", "scale", "stereo_close",
                            "stereo_bad_depth", "stereo_noisy")


def _pose34(R, O):
    """[R | t] with t = -R O, 3 x 4."""
    return np.concatenate([R, (-R @ O)[:, None]], 1)


def _pose34_inv(T):
    return np.concatenate([T[:, :3].T, (-T[:, :3].T @ T[:, 3])[:, None]], 1)


def make_new_map_points_scene(seed=0, kind="mono", npairs=4, cap=96, nfeat=(40, 96), cam=EUROC_CAM, mb=0.11, nlevels=8, scale_factor=1.2,
                              th_far=30.0, dense=False):
    """Keyframe pairs with known poses and points for CreateNewMapPoints: pair p = (image 2 p, image 2 p + 1), synthetic keypoints and a
    match table as SearchForTriangulation would leave it.  Even pairs move sideways, odd pairs forwards (low ray parallax near the axis,
    and points in front of keyframe 1 but behind keyframe 2).  Matches cycle through NEW_MAP_POINT_CATEGORIES, so that every way the
    reference's loop body ends occurs: points far away, behind the cameras, keypoints off by pixels, a far threshold, octaves that
    disagree with the distances, stereo features whose own parallax wins, stereo depths <= 0.  kind: "mono", "stereo1" / "stereo2"
    (stereo features in keyframe 1 / 2 only: mvuRight >= 0 and mvDepth), "rig" (KannalaBrandt8 pair, left then right features).
    A few idx2 are shared by two idx1.  dense: every feature of image 1 matched to a good point (the largest compaction).
    Returns a dict of numpy arrays; X [npairs, cap, 3] = the true point of each match (NaN where none), category [npairs, cap]."""
    assert kind in NEW_MAP_POINT_KINDS
    rng = np.random.default_rng(0x4E4D50 + 7919 * seed + NEW_MAP_POINT_KINDS.index(kind))
    rig = kind == "rig"
    nimg = 2 * npairs
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    mbf = fx * mb
    sf = np.array([scale_factor ** l for l in range(nlevels)], np.float32)
    sigma2 = (sf * sf).astype(np.float32)
    if rig:
        r28 = tumvi_rig28().astype(np.float64)
        camL8, camR8 = r28[:8], r28[8:16]
        Trl = np.concatenate([r28[16:25].reshape(3, 3), r28[25:28, None]], 1)
    else:
        camL8 = camR8 = np.array([fx, fy, cx, cy, 0, 0, 0, 0], np.float64)

    def project(side_right, Xc):
        if rig:
            return kb8_project(camR8 if side_right else camL8, Xc[None])[0]
        return np.array([fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy])

    def compose(Ta, Tb):   # Ta o Tb
        return np.concatenate([Ta[:, :3] @ Tb[:, :3], (Ta[:, :3] @ Tb[:, 3] + Ta[:, 3])[:, None]], 1)

    count = np.zeros(nimg, np.int32)
    nLeft = np.full(nimg, -1, np.int32)
    xy = rng.uniform([20, 20], [730, 460], (nimg, cap, 2))
    octave = rng.integers(0, nlevels, (nimg, cap)).astype(np.int32)
    desc = rng.integers(0, 256, (nimg, cap, 32), dtype=np.uint8)
    uRight = np.full((nimg, cap), -1.0, np.float32)
    depth = np.full((nimg, cap), -1.0, np.float32)
    match12 = np.full((npairs, cap), -1, np.int32)
    X = np.full((npairs, cap, 3), np.nan)
    category = np.full((npairs, cap), -1, np.int32)
    poses = np.zeros((npairs, 8 if rig else 4, 12), np.float32)
    kf2First = (rng.random(npairs) < 0.5).astype(np.uint8)
    cats = list(NEW_MAP_POINT_CATEGORIES)
    # what SearchForTriangulation reads besides: a vocabulary node per feature (a matched pair shares one), and per pinhole pair R12, t12
    # (T1w * Tw2) and the epipole of keyframe 1's centre in keyframe 2
    node = rng.integers(0, 40, (nimg, cap)).astype(np.int32)
    R12, t12, ep = np.zeros((npairs, 9), np.float32), np.zeros((npairs, 3), np.float32), np.zeros((npairs, 2), np.float32)
    for p in range(npairs):
        forward = p % 2 == 1
        n1, n2 = (cap, cap) if dense else (int(v) for v in rng.integers(nfeat[0], nfeat[1] + 1, 2))
        count[2 * p], count[2 * p + 1] = n1, n2
        R1 = _rot_from_rotvec(rng.normal(0, 0.04, 3))
        O1 = rng.uniform(-1, 1, 3)
        b = np.array([0.3, 0.05, 1.2]) if forward else np.array([rng.uniform(1.0, 1.5), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)])
        R2 = _rot_from_rotvec(rng.normal(0, 0.02, 3)) @ R1
        O2 = O1 + R1.T @ b
        # the float poses are the scene: everything below is computed from them
        T = [_pose34(R1, O1).astype(np.float32).astype(np.float64), _pose34(R2, O2).astype(np.float32).astype(np.float64)]
        if rig:
            TR = [compose(Trl, T[0]).astype(np.float32).astype(np.float64), compose(Trl, T[1]).astype(np.float32).astype(np.float64)]
            blocks = [T[0], _pose34_inv(T[0]), TR[0], _pose34_inv(TR[0]), T[1], _pose34_inv(T[1]), TR[1], _pose34_inv(TR[1])]
            nl1, nl2 = int(0.6 * n1), int(0.6 * n2)
            nLeft[2 * p], nLeft[2 * p + 1] = nl1, nl2
        else:
            blocks = [T[0], _pose34_inv(T[0]), T[1], _pose34_inv(T[1])]
            nl1, nl2 = n1, n2
        poses[p] = np.stack(blocks).reshape(len(blocks), 12)
        Rr = T[0][:, :3] @ T[1][:, :3].T
        R12[p], t12[p] = Rr.ravel(), T[0][:, 3] - Rr @ T[1][:, 3]
        C1 = T[1][:, :3] @ (-T[0][:, :3].T @ T[0][:, 3]) + T[1][:, 3]
        ep[p] = [fx * C1[0] / C1[2] + cx, fy * C1[1] / C1[2] + cy]
        nm = n1 if dense else int(rng.integers(min(n1, n2) // 2, min(n1, n2) - 2))
        idx1 = np.sort(rng.permutation(n1)[:nm])
        idx2 = rng.integers(0, n2, nm) if dense else rng.permutation(n2)[:nm]
        shared = set() if dense else {5, 17}     # match k reuses match k - 1's feature of image 2 (and its point)
        prev = None
        for k in range(nm):
            i1, i2 = int(idx1[k]), int(idx2[k])
            cat = "good" if dense or k % 3 == 0 else cats[(k // 3 * 2 + k % 3) % len(cats)]
            if k in shared and prev is not None:
                i2, cat = prev[0], prev[2]
            right1, right2 = rig and i1 >= nl1, rig and i2 >= nl2
            Ta, Tb = (TR[0] if right1 else T[0]), (TR[1] if right2 else T[1])
            stereo_side = {"stereo1": 1, "stereo2": 2}.get(kind, 0)
            if cat in ("stereo_close", "stereo_bad_depth") and not (stereo_side and forward):
                cat = "good"
            if cat == "stereo_noisy" and not stereo_side:
                cat = "good"
            if cat in ("behind_both", "behind_2") and rig:
                cat = "good"
            if cat == "behind_2" and not forward:
                cat = "behind_both"
            if cat == "far" and forward:
                cat = "good"
            o1 = int(rng.integers(0, 4)); o2 = o1
            sgn = rng.choice([-1.0, 1.0], 2)
            tx, ty = sgn[0] * rng.uniform(0.25, 0.55), sgn[1] * rng.uniform(0.1, 0.35)
            z = rng.uniform(4.0, 9.0)
            if cat == "low_parallax":
                z = 400.0
            elif cat == "behind_both":
                z = -6.0
            elif cat == "behind_2":
                tx, ty, z = 0.25, 0.1, 0.6
            elif cat == "far":
                z = rng.uniform(36.0, 45.0)
            elif cat in ("stereo_close", "stereo_bad_depth"):
                # next to the line of motion: the rays are almost parallel, the stereo feature's own parallax is the larger one
                tx, ty, z = b[0] / b[2] + rng.uniform(-0.002, 0.002), b[1] / b[2] + rng.uniform(-0.002, 0.002), rng.uniform(3.5, 5.0)
            elif cat == "scale":
                o1, o2 = 0, 4
            elif cat == "reproj1":
                o1 = o2 = 0
            elif cat == "reproj2":
                o1, o2 = 5, 0
            if k in shared and prev is not None:
                Xw = prev[1]
            else:
                Xa = np.array([tx * z, ty * z, z])
                Xw = Ta[:, :3].T @ (Xa - Ta[:, 3])
            Xa, Xb = Ta[:, :3] @ Xw + Ta[:, 3], Tb[:, :3] @ Xw + Tb[:, 3]
            if rig and (Xb[2] < 0.5 or Xa[2] < 0.5):
                continue   # (a KB8 camera does not see behind itself here: leave the feature unmatched)
            kpa, kpb = project(right1, Xa), project(right2, Xb)
            if cat in ("reproj1", "reproj2") and not (k in shared and prev is not None):
                # off the epipolar line by 8 px (6 px in image 2): the line through the keypoint and the image of a point moved towards
                # the other camera's centre
                Oa, Ob = -Ta[:, :3].T @ Ta[:, 3], -Tb[:, :3].T @ Tb[:, 3]
                if cat == "reproj1":
                    d = project(right1, Xa + 0.05 * (Ta[:, :3] @ (Ob - Xw))) - kpa
                    kpa = kpa + 8.0 * np.array([-d[1], d[0]]) / np.linalg.norm(d)
                else:
                    d = project(right2, Xb + 0.05 * (Tb[:, :3] @ (Oa - Xw))) - kpb
                    kpb = kpb + 6.0 * np.array([-d[1], d[0]]) / np.linalg.norm(d)
            xy[2 * p, i1], octave[2 * p, i1] = kpa, o1
            if not (k in shared and prev is not None):
                xy[2 * p + 1, i2], octave[2 * p + 1, i2] = kpb, o2
            if stereo_side and (cat in ("stereo_close", "stereo_bad_depth", "stereo_noisy") or rng.random() < 0.6):
                img, i, Xs, kps_ = (2 * p, i1, Xa, kpa) if stereo_side == 1 else (2 * p + 1, i2, Xb, kpb)
                if Xs[2] > 0 and not (stereo_side == 2 and k in shared):
                    uRight[img, i] = kps_[0] - mbf / Xs[2] + (10.0 if cat == "stereo_noisy" else 0.0)
                    depth[img, i] = -1.0 if cat == "stereo_bad_depth" else Xs[2]
                    if uRight[img, i] < 0:
                        uRight[img, i], depth[img, i] = -1.0, -1.0
            match12[p, i1] = i2
            flips = (1 << rng.integers(0, 8, 32)).astype(np.uint8) * (rng.random(32) < 0.08)
            if k in shared and prev is not None:
                desc[2 * p, i1] = desc[2 * p + 1, i2] ^ flips
                node[2 * p, i1] = node[2 * p + 1, i2]
            else:
                desc[2 * p + 1, i2] = desc[2 * p, i1] ^ flips
                node[2 * p + 1, i2] = node[2 * p, i1]
            X[p, i1] = Xw
            category[p, i1] = cats.index(cat)
            prev = (i2, Xw, cat)
    return dict(kind=kind, rig=rig, npairs=npairs, nimg=nimg, cap=cap, count=count, nLeft=nLeft, xy=xy.astype(np.float32),
                # mvKeys beside mvKeysUn: a fixed offset stands for the undistortion (read by UnprojectStereo only)
                xyRaw=(xy + np.array([0.3, -0.2])).astype(np.float32), octave=octave, desc=desc, uRight=uRight, depth=depth,
                node=node, R12=R12, t12=t12, ep=ep, match12=match12, img1=np.arange(0, nimg, 2, dtype=np.int32), img2=np.arange(1, nimg, 2, dtype=np.int32), poses=poses,
                kf2First=kf2First, X=X, category=category, scaleFactors=sf, levelSigma2=sigma2, camL8=camL8.astype(np.float32),
                camR8=camR8.astype(np.float32), cam=dict(fx=fx, fy=fy, cx=cx, cy=cy), mb=float(mb), mbf=float(mbf),
                ratioFactor=float(np.float32(1.5) * np.float32(scale_factor)), inertial=kind in ("stereo1", "rig"), farPoints=True,
                thFarPoints=float(th_far), width=752, height=480)


def new_map_points_frame_params(scene):
    from .capi import make_frame_params
    c = scene["cam"]
    return make_frame_params(scene["width"], scene["height"], c["fx"], c["fy"], c["cx"], c["cy"], scene["mbf"], scene["mb"],
                             [float(v) for v in scene["scaleFactors"]], [float(v) for v in scene["levelSigma2"]])


def pack_new_map_points_scene(scene, device):
    """make_new_map_points_scene -> the torch tensors of ORBmatcher.CreateNewMapPoints on `device` (kps / kpsRaw as u8 views of KP_DTYPE
    records [nimg, cap]; uRight / depth None for the kinds without stereo features; hasMP zeros)."""
    import torch
    from .capi import KP_DTYPE
    nimg, cap = scene["nimg"], scene["cap"]

    def records(xy):
        k = np.zeros((nimg, cap), KP_DTYPE)
        k["x"], k["y"], k["size"], k["octave"] = xy[..., 0], xy[..., 1], 31.0, scene["octave"]
        return torch.from_numpy(k.view(np.uint8).reshape(nimg, cap, KP_DTYPE.itemsize).copy()).to(device)
    stereo = scene["kind"] in ("stereo1", "stereo2")
    t = {k: torch.from_numpy(np.ascontiguousarray(scene[k])).to(device) for k in ("count", "desc", "match12", "img1", "img2")}
    t.update(kps=records(scene["xy"]), kpsRaw=records(scene["xyRaw"]) if stereo else None,
             uRight=torch.from_numpy(scene["uRight"]).to(device) if stereo else None,
             depth=torch.from_numpy(scene["depth"]).to(device) if stereo else None,
             nLeft1=torch.from_numpy(scene["nLeft"][scene["img1"]].copy()).to(device) if scene["rig"] else None,
             nLeft2=torch.from_numpy(scene["nLeft"][scene["img2"]].copy()).to(device) if scene["rig"] else None,
             hasMP=torch.zeros((nimg, cap), dtype=torch.uint8, device=device),
             row=torch.arange(scene["npairs"], dtype=torch.int32).to(device))
    return t


def make_local_mapping_scene(seed=0, B=2, K=3, cap=128, npts=100, cam=EUROC_CAM, mb=0.11, nlevels=8, scale_factor=1.2):
    """B new keyframes with K neighbours each for the local-mapping chain (search, create, Fuse per neighbour rank): image b (K + 1) is
    current keyframe b, the K images behind it are its neighbours by rank.  Every current keyframe sees npts points; each neighbour
    sees about two thirds of them at features of its own, so that a point is matched in several ranks and only the first creates it;
    five features of a current keyframe are there twice, so that two idx1 share one idx2.
    Pinhole, monocular.  Returns the pool (count, xy, octave, desc, node) and per rank k and keyframe b: img1 [B], img2 [K, B], R12,
    t12, ep, poses [K, B, 4, 12], kf2First [K, B], and the neighbour's pose as Fuse takes it: Tcw7 [K, B, 7], Ow [K, B, 3]."""
    rng = np.random.default_rng(0x4C4D43 + seed)
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    nimg = B * (K + 1)
    sf = np.array([scale_factor ** l for l in range(nlevels)], np.float32)
    count = np.zeros(nimg, np.int32)
    xy = rng.uniform([20, 20], [730, 460], (nimg, cap, 2))
    octave = np.zeros((nimg, cap), np.int32)
    desc = rng.integers(0, 256, (nimg, cap, 32), dtype=np.uint8)
    node = rng.integers(0, 40, (nimg, cap)).astype(np.int32)
    img2 = np.zeros((K, B), np.int32)
    R12, t12, ep = np.zeros((K, B, 9), np.float32), np.zeros((K, B, 3), np.float32), np.zeros((K, B, 2), np.float32)
    poses, kf2First = np.zeros((K, B, 4, 12), np.float32), (rng.random((K, B)) < 0.5).astype(np.uint8)
    Tcw7, Ow = np.zeros((K, B, 7), np.float32), np.zeros((K, B, 3), np.float32)
    for b in range(B):
        c = b * (K + 1)
        R1, O1 = _rot_from_rotvec(rng.normal(0, 0.03, 3)), rng.uniform(-1, 1, 3)
        T1 = _pose34(R1, O1).astype(np.float32).astype(np.float64)
        count[c] = npts + 10
        Xc = np.stack([rng.uniform(-0.5, 0.5, npts), rng.uniform(-0.3, 0.3, npts), np.ones(npts)], 1) * rng.uniform(4, 9, (npts, 1))
        Xw = (Xc - T1[:, 3]) @ T1[:, :3]
        xy[c, :npts] = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
        octave[c, :npts] = rng.integers(0, 3, npts)
        # five features twice in the current keyframe: both copies match the same feature of a neighbour (a shared idx2)
        for a in (xy, octave, desc, node):
            a[c, npts:npts + 5] = a[c, :5]
        for k in range(K):
            j = c + 1 + k
            img2[k, b] = j
            ang = 2 * np.pi * k / K + 0.3
            O2 = O1 + R1.T @ np.array([1.2 * np.cos(ang), 1.2 * np.sin(ang), rng.uniform(-0.1, 0.1)])
            T2 = _pose34(_rot_from_rotvec(rng.normal(0, 0.02, 3)) @ R1, O2).astype(np.float32).astype(np.float64)
            seen = np.nonzero(rng.random(npts) < 0.66)[0]
            slot = rng.permutation(npts + 10)[:len(seen)]
            count[j] = npts + 10
            X2 = Xw[seen] @ T2[:, :3].T + T2[:, 3]
            xy[j, slot] = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1)
            octave[j, slot] = octave[c, seen]
            flips = (1 << rng.integers(0, 8, (len(seen), 32))).astype(np.uint8) * (rng.random((len(seen), 32)) < 0.08)
            desc[j, slot] = desc[c, seen] ^ flips
            node[j, slot] = node[c, seen]
            Rr = T1[:, :3] @ T2[:, :3].T
            R12[k, b], t12[k, b] = Rr.ravel(), T1[:, 3] - Rr @ T2[:, 3]
            C1 = T2[:, :3] @ O1 + T2[:, 3]
            ep[k, b] = [fx * C1[0] / C1[2] + cx, fy * C1[1] / C1[2] + cy]
            poses[k, b] = np.stack([T1, _pose34_inv(T1), T2, _pose34_inv(T2)]).reshape(4, 12)
            Tcw7[k, b] = np.concatenate([_quat_from_R(T2[:, :3]), T2[:, 3]])
            Ow[k, b] = _pose34_inv(T2)[:, 3]
    return dict(kind="mono", rig=False, B=B, K=K, nimg=nimg, cap=cap, count=count, xy=xy.astype(np.float32), octave=octave, desc=desc, node=node,
                img1=np.arange(0, nimg, K + 1, dtype=np.int32), img2=img2, R12=R12, t12=t12, ep=ep, poses=poses, kf2First=kf2First, Tcw7=Tcw7,
                Ow=Ow, scaleFactors=sf, levelSigma2=(sf * sf).astype(np.float32), cam=dict(fx=fx, fy=fy, cx=cx, cy=cy), mb=float(mb),
                mbf=float(fx * mb), ratioFactor=float(np.float32(1.5) * np.float32(scale_factor)), width=752, height=480)


# ---- CreateInitialMapMonocular (the two frames of a monocular initialisation behind TwoViewReconstruction) ----------------------
def make_initial_map_problem(seed=0, n_points=150, n_extra=(20, 15), n_untriangulated=6, cam="pinhole", depth=(2.5, 9.0), baseline=0.4,
                             noise_px=0.5, outlier_frac=0.0, point_noise=0.03, pose_noise=(0.01, 0.03), nlevels=8, scale_factor=1.2,
                             behind=False, width=752, height=480):
    """One input of morb_create_initial_map_monocular_batch as the two upstream entries would leave it, seeded.  Keyframe 1 sits at the
    origin and sees n_points points in the depth slab `depth` (behind=True: the slab lies behind the camera, so that the median depth is
    negative); keyframe 2 sits `baseline` away.  Every point is observed in both frames with Gaussian pixel noise noise_px * 1.2^octave
    (the octave drawn per keypoint), a share outlier_frac of the frame-2 observations is moved by 25 .. 80 pixels.  n_extra unmatched
    keypoints per frame and n_untriangulated matched ones that TwoViewReconstruction left out (triangulated 0) are mixed in, in a seeded
    order.  cam: "pinhole" (EuRoC) or "kb8" (TUM-VI left).  P3D and T21 are the truth moved by point_noise (relative) and pose_noise
    (rotation in radians, translation relative to the baseline).  Returns kp1 / kp2 (x, y, octave) f32 [n1 / n2, 3], matches12 i32 [n1],
    triangulated u8 [n1], P3D f32 [n1, 3], T21 f32 [12] (R row-major, t), ok, cam8 f32 [8], kb8, scaleFactors / levelSigma2 f32 [nlevels],
    and the truth T21_true f64 [12], X_true f64 [n1, 3]."""
    assert cam in ("pinhole", "kb8")
    rng = np.random.default_rng(0x1A17 + seed)
    kb8 = cam == "kb8"
    c8 = TUMVI_CAM_L.astype(np.float32) if kb8 else np.array([EUROC_CAM[k] for k in ("fx", "fy", "cx", "cy")] + [0, 0, 0, 0], np.float32)
    w, h = (512, 512) if kb8 else (width, height)
    sf = np.float32(scale_factor) ** np.arange(nlevels, dtype=np.float32)
    m = n_points + n_untriangulated
    n1, n2 = m + n_extra[0], m + n_extra[1]

    def proj(X):
        if kb8:
            return kb8_project(c8.astype(np.float64), X)
        return np.stack([c8[0] * X[:, 0] / X[:, 2] + c8[2], c8[1] * X[:, 1] / X[:, 2] + c8[3]], 1)

    def backproject(u, z):
        if not kb8:
            return np.stack([(u[:, 0] - c8[2]) / c8[0] * z, (u[:, 1] - c8[3]) / c8[1] * z, z], 1)
        # a ray per pixel by bisection on theta (the polynomial is monotonic over the field of view)
        px, py = (u[:, 0] - c8[2]) / c8[0], (u[:, 1] - c8[3]) / c8[1]
        rd = np.sqrt(px * px + py * py)
        lo, hi = np.zeros_like(rd), np.full_like(rd, 1.5)
        for _ in range(60):
            th = 0.5 * (lo + hi)
            f = th + c8[4] * th ** 3 + c8[5] * th ** 5 + c8[6] * th ** 7 + c8[7] * th ** 9
            lo, hi = np.where(f < rd, th, lo), np.where(f < rd, hi, th)
        th = 0.5 * (lo + hi)
        s = np.where(rd > 1e-12, np.tan(th) / np.maximum(rd, 1e-12), 1.0)
        return np.stack([px * s * z, py * s * z, z], 1)

    margin = 0.22 if kb8 else 0.06
    u1 = np.stack([rng.uniform(margin * w, (1 - margin) * w, m), rng.uniform(margin * h, (1 - margin) * h, m)], 1)
    z = rng.uniform(depth[0], depth[1], m) * (-1.0 if behind else 1.0)
    X = backproject(u1, z)
    R = _rot_from_rotvec(rng.normal(0, 0.04, 3))
    tdir = np.array([rng.choice([-1.0, 1.0]) * rng.uniform(0.8, 1.0), rng.normal(0, 0.2), rng.normal(0, 0.1)])
    t = tdir / np.linalg.norm(tdir) * baseline
    X2 = X @ R.T + t
    u2 = proj(X2)
    oct1, oct2 = rng.integers(0, nlevels, n1), rng.integers(0, nlevels, n2)
    i1 = np.sort(rng.permutation(n1)[:m])
    i2 = rng.permutation(n2)[:m]
    kp1 = np.stack([rng.uniform(0, w, n1), rng.uniform(0, h, n1), oct1], 1)
    kp2 = np.stack([rng.uniform(0, w, n2), rng.uniform(0, h, n2), oct2], 1)
    kp1[i1, :2] = u1 + rng.normal(0, 1, (m, 2)) * (noise_px * sf[oct1[i1]])[:, None]
    kp2[i2, :2] = u2 + rng.normal(0, 1, (m, 2)) * (noise_px * sf[oct2[i2]])[:, None]
    out = rng.random(m) < outlier_frac
    ang = rng.uniform(0, 2 * np.pi, m)
    kp2[i2[out], :2] += (rng.uniform(25, 80, m)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1))[out]
    matches = np.full(n1, -1, np.int32)
    matches[i1] = i2
    tri = np.zeros(n1, np.uint8)
    keep = np.ones(m, bool)
    keep[rng.permutation(m)[:n_untriangulated]] = False
    tri[i1[keep]] = 1
    P3D = np.zeros((n1, 3), np.float32)
    P3D[i1[keep]] = (X * (1 + rng.normal(0, point_noise, (m, 1))) + rng.normal(0, point_noise * 0.2, (m, 3)))[keep]
    Xt = np.zeros((n1, 3))
    Xt[i1[keep]] = X[keep]
    Rn = _rot_from_rotvec(rng.normal(0, pose_noise[0], 3)) @ R
    tn = t + rng.normal(0, pose_noise[1], 3) * baseline
    return dict(n1=n1, n2=n2, kp1=kp1.astype(np.float32), kp2=kp2.astype(np.float32), matches12=matches, triangulated=tri, P3D=P3D,
                T21=np.concatenate([Rn.ravel(), tn]).astype(np.float32), ok=1, cam8=c8, kb8=int(kb8), scaleFactors=sf,
                levelSigma2=(sf * sf).astype(np.float32), nlevels=nlevels, width=w, height=h, T21_true=np.concatenate([R.ravel(), t]), X_true=Xt,
                outlier=out)


def initial_map_frame_params(prob):
    from .capi import make_frame_params
    c = prob["cam8"]
    return make_frame_params(prob["width"], prob["height"], float(c[0]), float(c[1]), float(c[2]), float(c[3]), 0.0, 0.0,
                             [float(v) for v in prob["scaleFactors"]], [float(v) for v in prob["levelSigma2"]])


def pack_initial_map_problems(probs, device, cap=None):
    """make_initial_map_problem dicts -> the torch tensors of Optimizer.CreateInitialMapMonocular on `device`: a keypoint pool kps (u8 view
    of KP_DTYPE records [2 P, cap]; problem p owns images 2 p and 2 p + 1), img1 / img2 i32 [P], count i32 [2 P], matches12 i32 [P, cap]
    (-1 padded), ok i32 [P], T21 f32 [P, 12], P3D f32 [P, cap, 3], triangulated u8 [P, cap].  cap = the largest frame unless given."""
    import torch
    from .capi import KP_DTYPE
    P = len(probs)
    cap = cap or max(max(max(p["n1"], p["n2"]) for p in probs), 1)
    kps = np.zeros((2 * P, cap), KP_DTYPE)
    count = np.zeros(2 * P, np.int32)
    m12 = np.full((P, cap), -1, np.int32)
    tri = np.zeros((P, cap), np.uint8)
    P3D = np.zeros((P, cap, 3), np.float32)
    for k, p in enumerate(probs):
        for j, (key, n) in enumerate((("kp1", p["n1"]), ("kp2", p["n2"]))):
            r = kps[2 * k + j, :n]
            r["x"], r["y"], r["octave"], r["size"] = p[key][:, 0], p[key][:, 1], p[key][:, 2].astype(np.int32), 31.0
            count[2 * k + j] = n
        m12[k, :p["n1"]] = p["matches12"]
        tri[k, :p["n1"]] = p["triangulated"]
        P3D[k, :p["n1"]] = p["P3D"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return {"kps": t(kps.view(np.uint8).reshape(2 * P, cap, KP_DTYPE.itemsize).copy()), "img1": t(np.arange(0, 2 * P, 2, dtype=np.int32)),
            "img2": t(np.arange(1, 2 * P, 2, dtype=np.int32)), "count": t(count), "matches12": t(m12), "triangulated": t(tri), "P3D": t(P3D),
            "ok": t(np.array([p["ok"] for p in probs], np.int32)), "T21": t(np.stack([p["T21"] for p in probs]).astype(np.float32))}


# ---- map merging: the welding bundle adjustment (Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag)) ----------
def make_merge_ba_problem(n_free=25, n_fixed=25, n_points=3500, seed=0, mono_frac=0.3, kb8=False, outlier_frac=0.04, rigid_deg=0.6,
                          rigid_trans=0.03, kf_deg=0.15, kf_trans=0.005, point_noise=0.02, noise_px=1.0, obs_per_point=(4, 11), bad_points=0,
                          bad_kf=None, stuck_kf=None, stuck_deg=2.5, stuck_trans=0.08, kf_edges=None, cam=EUROC_CAM):
    """Input of the welding BA of LoopClosing::MergeLocal: a free window (keyframes 0 .. n_free - 1, vpAdjustKF) and a fixed window (the
    matched map's, vpFixedKF) on one arc looking at common points.  The free window is displaced rigidly by what a Sim3 alignment leaves
    (rigid_deg, rigid_trans), each of its keyframes by a little more (kf_deg, kf_trans); a fraction of the observations are gross
    outliers (wrong fusions).  mono_frac: the share of monocular observations (1.0: none stereo); kb8: every observation monocular on the
    TUM-VI left KannalaBrandt8 camera (eObs is [nE, 2], `camL` the camera).  bad_points: that many points have ONLY gross observations;
    bad_kf: a free keyframe whose observations are ALL gross; stuck_kf: a free keyframe with a pose error of its own (stuck_deg,
    stuck_trans) that a few robust iterations do not remove; kf_edges = {keyframe: count}: that keyframe observes exactly `count` points."""
    rng = np.random.default_rng(0x3E26E + seed)
    nkf = n_free + n_fixed
    poses = []
    for i in range(nkf):
        ang = (i / max(nkf - 1, 1) - 0.5) * 0.5
        c = np.array([2.0 * np.sin(ang) * 2, rng.normal(0, 0.05), -2.0 * (1 - np.cos(ang))])
        q_wc = _quat_from_rotvec(np.array([0, -ang * 0.8, 0]) + rng.normal(0, 0.01, 3))
        q_cw = q_wc * np.array([-1, -1, -1, 1])
        poses.append(np.concatenate([q_cw, -_quat_rot(q_cw, c)]))
    poses = np.array(poses)
    zr = (2.0, 8.0) if kb8 else (3.0, 10.0)
    X = np.stack([rng.uniform(-3, 3, n_points), rng.uniform(-2, 2, n_points), rng.uniform(*zr, n_points)], 1)

    def observe(kf, j):
        """(observation, 1 / sigma^2) of point j in keyframe kf, or None when it is not in the image"""
        Xc = _quat_rot(poses[kf][:4], X[j]) + poses[kf][4:]
        if kb8:
            if Xc[2] <= 0.4:
                return None
            uv = kb8_project(TUMVI_CAM_L, Xc[None])[0]
            if not (5 < uv[0] < 507 and 5 < uv[1] < 507):
                return None
            o = uv
        else:
            if Xc[2] <= 0.5:
                return None
            u = cam["fx"] * Xc[0] / Xc[2] + cam["cx"]; v = cam["fy"] * Xc[1] / Xc[2] + cam["cy"]
            if not (0 <= u < 752 and 0 <= v < 480):
                return None
            o = np.array([u, v, u - cam["bf"] / Xc[2]])
        s = 1.2 ** int(rng.integers(0, 8))
        o = o + rng.normal(0, noise_px, len(o)) * s
        if not kb8 and rng.random() < mono_frac:
            o[2] = -1
        return o, 1.0 / s ** 2

    fixed_count = dict(kf_edges or {})
    seen = set()
    eKF, eMP, eObs, eInv = [], [], [], []
    for j in range(n_points):
        k = int(rng.integers(*obs_per_point))
        for kf in rng.choice(nkf, size=min(k, nkf), replace=False):
            if int(kf) in fixed_count:
                continue
            r = observe(int(kf), j)
            if r is not None:
                eKF.append(int(kf)); eMP.append(j); eObs.append(r[0]); eInv.append(r[1]); seen.add((int(kf), j))
    for kf, count in fixed_count.items():
        got = 0
        for j in rng.permutation(n_points):
            if got == count:
                break
            r = observe(kf, int(j))
            if r is not None:
                eKF.append(kf); eMP.append(int(j)); eObs.append(r[0]); eInv.append(r[1]); got += 1
        assert got == count, (kf, got, count)
    eKF, eMP, eObs, eInv = np.array(eKF, np.int32), np.array(eMP, np.int32), np.array(eObs, np.float64), np.array(eInv, np.float32)
    order = np.lexsort((eKF, eMP))          # (edges by point, as the reference walks its points' observations)
    eKF, eMP, eObs, eInv = eKF[order], eMP[order], eObs[order], eInv[order]
    gross = rng.random(len(eKF)) < outlier_frac
    if bad_points:
        gross |= np.isin(eMP, rng.choice(n_points, bad_points, replace=False))
    if bad_kf is not None:
        gross |= eKF == bad_kf
    off = rng.choice([-1, 1], (len(eKF), 2)) * rng.uniform(15, 30, (len(eKF), 2))
    eObs[gross, :2] += off[gross]
    # the free window: a rigid displacement of the whole window in the world, then per-keyframe noise
    dq = _quat_from_rotvec(rng.normal(0, 1, 3) / np.sqrt(3) * np.deg2rad(rigid_deg))
    dt = rng.normal(0, 1, 3) / np.sqrt(3) * rigid_trans
    pose0 = poses.copy()
    for i in range(n_free):
        q = _quat_mul(poses[i][:4], dq)                                    # Tcw' = Tcw * D,  D = (dq, dt) acting on the world
        t = _quat_rot(poses[i][:4], dt) + poses[i][4:]
        deg, tr = (stuck_deg, stuck_trans) if i == stuck_kf else (kf_deg, kf_trans)
        nq = _quat_from_rotvec(rng.normal(0, 1, 3) / np.sqrt(3) * np.deg2rad(deg))
        pose0[i] = np.concatenate([_quat_mul(nq, q), _quat_rot(nq, t) + rng.normal(0, 1, 3) / np.sqrt(3) * tr])
    X0 = X + rng.normal(0, point_noise, X.shape)
    fixed = np.zeros(nkf, np.uint8); fixed[n_free:] = 1
    out = dict(kfPose=pose0.astype(np.float32), kfFixed=fixed, mpPos=X0.astype(np.float32), eKF=eKF, eMP=eMP, eInvSigma2=eInv,
               true_poses=poses, true_points=X, gross=gross, cam=cam, camL=None)
    if kb8:
        out.update(eObs=eObs[:, :2].astype(np.float32), camL=TUMVI_CAM_L)
    else:
        out["eObs"] = eObs.astype(np.float32)
    return out


# ---- map merging with an IMU: Optimizer::MergeInertialBA(pCurrKF, pMergeKF, pbStopFlag, pMap, corrPoses) ------------------------------
def make_merge_inertial_ba_problem(n_cur=5, n_merge=5, n_cov=4, n_points=300, seed=0, mono_frac=0.3, kb8=False, n_imu=40, n_fixed_vis=0,
                                   outlier_frac=0.03, rigid_deg=0.3, rigid_trans=0.02, kf_deg=0.3, kf_trans=0.01, point_noise=0.03,
                                   obs_per_point=(3, 9), noise_px=1.0, vel_noise=0.03, bias_noise=1.0, kf_edges=None, vel_kick=None, fixed_shift=0.0, fixed_pair=0.0,
                                   n_behind=0,
                                   n_cov_only=0, cam=EUROC_CAM):
    """MergeInertialBA input (morb_merge_inertial_ba): chain A, the current map's window — one free head (vpOptimizableCovKFs[0]) then
    n_cur free keyframes; chain B, the merge map's window — one fixed keyframe with an IMU state (lFixedKeyFrames) then n_merge free
    keyframes; n_cov keyframes free in the pose only and n_fixed_vis fixed observers, all looking at the same points.  kfKind 0 / 1 / 2 /
    3 as the entry takes them; every link carries n_imu IMU samples of a smooth motion as in make_inertial_ba_problem.  Chain A starts
    displaced rigidly by what the Sim3 alignment leaves (rigid_deg, rigid_trans), every free keyframe by a little more.  kb8: every
    observation monocular on the left camera of the TUM-VI rig (`rig28`).  Knobs: kf_edges = {keyframe: count}: that keyframe observes
    exactly `count` points; vel_kick = {keyframe: m/s}: its initial velocity is off by that much (a link whose chi2 starts above the Huber
    bar); fixed_shift: the fixed keyframe of chain B stands that many metres off along every axis; fixed_pair: chain B begins with TWO
    fixed keyframes with an IMU state joined by a link, the first of them (which observes nothing) that many metres off — a link between
    fixed vertices, a constant of the robust chi2 that no step changes; n_behind: extra points BEHIND every camera whose monocular
    observations agree with them (a negative depth with a small chi2);
    n_cov_only: extra points seen by pose-only keyframes alone; noise_px, vel_noise, bias_noise (a factor): the observation noise and
    the initial error of the free keyframes' velocities and biases (all zero with the displacements: the graph starts at its optimum)."""
    rng = np.random.default_rng(0x41BA0 + seed)
    g = np.array([0, 0, -9.81])
    dt = 1.0 / IMU_FREQ
    bg = rng.normal(0, 0.01, 3); ba = rng.normal(0, 0.05, 3)
    Tbc = EUROC_TBC
    Rcb = Tbc[:3, :3].T; tcb = -Rcb @ Tbc[:3, 3]
    acc, gyro, dts, start = [], [], [], [0]
    states, iKF1, iKF2 = [], [], []

    def chain(n_links, R, p, v):
        states.append((R, p, v))
        for _ in range(n_links):
            w_b = rng.normal(0, 0.15, 3); a_w = rng.normal(0, 0.5, 3)
            for i in range(n_imu):
                Rm = R @ _rot_from_rotvec(w_b * (i + 0.5) * dt)
                acc.append(Rm.T @ (a_w - g) + ba + rng.normal(0, 0.02, 3))
                gyro.append(w_b + bg + rng.normal(0, 0.002, 3))
                dts.append(dt)
            T = n_imu * dt
            R, p, v = R @ _rot_from_rotvec(w_b * T), p + v * T + 0.5 * a_w * T * T, v + a_w * T
            iKF1.append(len(states) - 1); iKF2.append(len(states))
            states.append((R, p, v))
            start.append(len(dts))

    R0 = _rot_from_rotvec(rng.normal(0, 0.1, 3)); p0 = rng.normal(0, 0.2, 3)
    chain(n_cur, R0, p0, np.array([0.6, 0.1, 0.0]) + rng.normal(0, 0.1, 3))
    nA = len(states)
    nFix = 2 if fixed_pair else 1
    chain(n_merge + nFix - 1, R0 @ _rot_from_rotvec(rng.normal(0, 0.05, 3)), p0 + rng.normal(0, 0.25, 3), np.array([0.5, -0.1, 0.0]) + rng.normal(0, 0.1, 3))
    nChain = len(states)
    for _ in range(n_cov + n_fixed_vis):
        Rk, pk, _ = states[rng.integers(0, nChain)]
        states.append((Rk @ _rot_from_rotvec(rng.normal(0, 0.05, 3)), pk + rng.normal(0, 0.15, 3), rng.normal(0, 0.3, 3)))
    nKF = len(states)
    kind = np.array([0] * nA + [1] * nFix + [0] * n_merge + [3] * n_cov + [2] * n_fixed_vis, np.uint8)
    cams = [(Rcb @ Rk.T, Rcb @ (-Rk.T @ pk) + tcb) for Rk, pk, _ in states]
    Rm, tm_ = cams[nA // 2]
    zr = (2.0, 8.0) if kb8 else (2.0, 20.0)
    n_all = n_points + n_behind + n_cov_only
    Xc = np.stack([rng.uniform(-4, 4, n_all), rng.uniform(-2.5, 2.5, n_all), rng.uniform(*zr, n_all)], 1)
    Xc[n_points:n_points + n_behind, 2] = -rng.uniform(3, 8, n_behind)
    X = (Xc - tm_) @ Rm

    def observe(k, j, mono=False):
        """(observation x y uRight, 1 / sigma^2) of point j in keyframe k, or None when it is not in the image"""
        Rcw, tcw = cams[k]
        xc = Rcw @ X[j] + tcw
        behind = n_points <= j < n_points + n_behind
        if (xc[2] < 0.5) != behind or abs(xc[2]) < 0.5:
            return None
        s = 1.2 ** int(rng.integers(0, 8))
        if kb8:
            u, vv = kb8_project(TUMVI_CAM_L, xc[None])[0]
            if not behind and not (5 < u < 507 and 5 < vv < 507):
                return None
            s *= 0.5
            o = np.array([u, vv, -1.0]) + np.array([rng.normal(0, noise_px) * s, rng.normal(0, noise_px) * s, 0.0])
        else:
            u = cam["fx"] * xc[0] / xc[2] + cam["cx"]; vv = cam["fy"] * xc[1] / xc[2] + cam["cy"]
            if not behind and not (0 <= u < 752 and 0 <= vv < 480):
                return None
            o = np.array([u, vv, u - cam["bf"] / xc[2]]) + rng.normal(0, noise_px, 3) * s
            if mono or behind or rng.random() < mono_frac:
                o[2] = -1
        return o, 1.0 / (s * s)

    counted = dict(kf_edges or {})
    if fixed_pair:
        counted[nA] = 0
    cov = [k for k in range(nKF) if kind[k] == 3]
    assert not n_cov_only or len(cov) >= 2
    eKF, eMP, eObs, eInv = [], [], [], []
    for j in range(n_all):
        pool = cov if j >= n_points + n_behind else list(range(nKF))
        for k in rng.choice(pool, size=min(int(rng.integers(*obs_per_point)), len(pool)), replace=False):
            if int(k) in counted:
                continue
            r = observe(int(k), j)
            if r is not None:
                eKF.append(int(k)); eMP.append(j); eObs.append(r[0]); eInv.append(r[1])
    for k, count in counted.items():
        got = 0
        for j in rng.permutation(n_points):
            if got == count:
                break
            r = observe(k, int(j))
            if r is not None:
                eKF.append(k); eMP.append(int(j)); eObs.append(r[0]); eInv.append(r[1]); got += 1
        assert got == count, (k, got, count)
    eKF, eMP, eObs, eInv = np.array(eKF, np.int32), np.array(eMP, np.int32), np.array(eObs, np.float64), np.array(eInv, np.float32)
    order = np.lexsort((eKF, eMP))          # (edges by point, as the reference walks its points' observations)
    eKF, eMP, eObs, eInv = eKF[order], eMP[order], eObs[order], eInv[order]
    gross = (rng.random(len(eKF)) < outlier_frac) & (eMP < n_points)
    off = rng.choice([-1, 1], (len(eKF), 2)) * rng.uniform(15, 30, (len(eKF), 2))
    eObs[gross, :2] += off[gross]
    # every point is seen: points nobody observes are dropped (the reference builds its points from the keyframes' matches)
    used = np.zeros(n_all, bool); used[eMP] = True
    remap = np.cumsum(used) - 1
    eMP = remap[eMP].astype(np.int32)
    tags = np.zeros(n_all, np.uint8); tags[n_points:n_points + n_behind] = 1; tags[n_points + n_behind:] = 2
    X, tags = X[used], tags[used]
    true = np.stack([np.concatenate([Rk.ravel(), pk, vk, bg, ba]) for Rk, pk, vk in states])
    init = true.copy()
    DR = _rot_from_rotvec(rng.normal(0, 1, 3) / np.sqrt(3) * np.deg2rad(rigid_deg)); Dt = rng.normal(0, 1, 3) / np.sqrt(3) * rigid_trans
    for k in range(nKF):
        if kind[k] in (1, 2):
            continue
        Rk, pk, vk = states[k]
        if k < nA:     # the current map's window, as the Sim3 alignment left it
            Rk, pk, vk = DR @ Rk, DR @ pk + Dt, DR @ vk
        Rk = Rk @ _rot_from_rotvec(rng.normal(0, 1, 3) / np.sqrt(3) * np.deg2rad(kf_deg))
        init[k, :9] = Rk.ravel(); init[k, 9:12] = pk + rng.normal(0, kf_trans, 3)
        if kind[k] == 0:
            init[k, 12:15] = vk + rng.normal(0, vel_noise, 3)
            init[k, 15:18] += rng.normal(0, 0.001, 3) * bias_noise; init[k, 18:21] += rng.normal(0, 0.005, 3) * bias_noise
    for k, dv in (vel_kick or {}).items():
        init[k, 12:15] += rng.normal(0, 1, 3) / np.sqrt(3) * dv
    init[nA + nFix - 1, 9:12] += fixed_shift          # (the fixed keyframe of chain B contradicts its link: trials get rejected)
    if fixed_pair:
        init[nA, 9:12] += fixed_pair
    out = dict(kfState=init.astype(np.float32), kfKind=kind, mpPos=(X + rng.normal(0, point_noise, X.shape)).astype(np.float32),
               mpTag=tags, eKF=eKF, eMP=eMP, eObs=eObs.astype(np.float32), eInvSigma2=eInv, iKF1=np.array(iKF1, np.int32),
               iKF2=np.array(iKF2, np.int32), imuStart=np.array(start, np.int32), acc=np.array(acc, np.float32),
               gyro=np.array(gyro, np.float32), dt=np.array(dts, np.float32), bias=np.concatenate([ba, bg]).astype(np.float32),
               Tbc12=np.concatenate([Tbc[:3, :3].ravel(), Tbc[:3, 3]]).astype(np.float32), cam=cam, true=true, truePts=X, gross=gross,
               rig28=tumvi_rig28() if kb8 else None)
    return out


# ---- the essential graph of loop closing (Optimizer::OptimizeEssentialGraph) ---------------------------------------------------------
def _sim3_mul(a, b):
    """g2o::Sim3::operator* on (qx qy qz qw tx ty tz s)."""
    return np.concatenate([_quat_mul(a[:4], b[:4]), a[7] * _quat_rot(a[:4], b[4:7]) + a[4:7], [a[7] * b[7]]])


def _sim3_inv(a):
    qc = np.array([-a[0], -a[1], -a[2], a[3]])
    return np.concatenate([qc, _quat_rot(qc, (-1.0 / a[7]) * a[4:7]), [1.0 / a[7]]])


def make_essential_graph_problem(n_kf=30, band=3, n_loop=1, fix_scale=False, seed=0, n_old_loops=0, loop_kf=1, loop_rot_deg=3.0,
                                 loop_trans=0.3, loop_scale=1.03, fixed=(0,), fix_scale_on=None, duplicate_every=0, fixed_pair_edge=False,
                                 isolated=(), n_points=0, drift_rot_deg=0.3, drift_scale=0.004, meas_noise=0.0, fixed_pair_offset=0.05):
    """A loop closure as LoopClosing::CorrectLoop hands it to Optimizer::OptimizeEssentialGraph, flattened for morb_optimize_essential_graph.
    Keyframes 0 .. n_kf-1 (ascending mnId) move along a drifting trajectory (per-step rotation and scale drift); keyframe i's parent is the
    nearest earlier keyframe that is not `isolated`; covisibility (weight >= 100) joins keyframes at most `band` apart.  The current keyframe
    is the last one, the loop keyframe `loop_kf`.  CorrectedSim3 / NonCorrectedSim3 are propagated as LoopClosing.cc:1105-1180 does: the
    current keyframe's corrected Sim3 is Sim3(loop error) * Scw, every keyframe connected to it (within `band`) gets Sic * corrected Scw, and
    its non-corrected Sim3 is its pose with s = 1.  Edges in the insertion order of Optimizer.cc:1514-1682 (vertex 0 = the later keyframe):
    the LoopConnections of the connected keyframes to the n_loop keyframes around the loop keyframe (measured between the ESTIMATES), then
    per keyframe its spanning-tree edge, its old loop edges (n_old_loops random long-range pairs), its covisibility edges and, every
    `duplicate_every`-th keyframe, an inertial edge that doubles the spanning-tree one; all measured between the NON-corrected poses.
    fixed: fixed vertices; fix_scale sets _fix_scale on all vertices (overload 1), fix_scale_on on those listed only (overload 2's shape).
    fixed_pair_edge adds an edge between two fixed vertices, its measurement off by fixed_pair_offset (a constant of chi2); `isolated` keyframes carry no edge.  Points: n_points with a reference
    keyframe each (every tenth -1).  Returns a dict: kfSim3, kfFlags, eI, eJ, eSji, mpPos, mpRef, plus cur, loop, connected, S_true."""
    rng = np.random.default_rng(seed)
    iso = set(int(i) for i in isolated)
    # true poses: a camera on a circle looking along its tangent; Scw with s = 1
    S_true = np.zeros((n_kf, 8))
    for i in range(n_kf):
        a = 2 * np.pi * i / max(n_kf, 8)
        q = _quat_from_rotvec(np.array([0.05 * np.sin(3 * a), -a, 0.03 * np.cos(2 * a)]))
        c = np.array([6 * np.cos(a), 0.2 * np.sin(5 * a), 6 * np.sin(a)])
        S_true[i] = np.concatenate([q, -_quat_rot(q, c), [1.0]])
    # drifted estimates (SE3: s = 1): the relative motions pick up a rotation and a scale error each
    S_est = np.zeros_like(S_true)
    S_est[0] = S_true[0]
    for i in range(1, n_kf):
        rel = _sim3_mul(S_true[i], _sim3_inv(S_true[i - 1]))
        dq = _quat_from_rotvec(np.deg2rad(drift_rot_deg) * (np.array([0.2, 1.0, 0.1]) + 0.3 * rng.normal(size=3)))
        rel = np.concatenate([_quat_mul(dq, rel[:4]), (1.0 - drift_scale * (1 + 0.3 * rng.normal())) * _quat_rot(dq, rel[4:7]), [1.0]])
        S_est[i] = _sim3_mul(rel, S_est[i - 1])
        S_est[i, :4] /= np.linalg.norm(S_est[i, :4])
    cur = n_kf - 1
    while cur in iso:
        cur -= 1
    connected = [i for i in range(max(0, cur - band), cur + 1) if i not in iso]
    # the loop error: Sim3(rotation, translation, scale) in front of the current keyframe's Scw
    lq = _quat_from_rotvec(np.deg2rad(loop_rot_deg) * np.array([0.3, 0.9, -0.2]) / np.linalg.norm([0.3, 0.9, -0.2]))
    G = np.concatenate([lq, loop_trans * np.array([0.5, -0.2, 0.8]), [1.0 if fix_scale else loop_scale]])
    S_cur_corr = _sim3_mul(G, S_est[cur])
    vS = S_est.copy()   # vScw: CorrectedSim3's entry, or the pose
    for i in connected:
        Sic = _sim3_mul(S_est[i], _sim3_inv(S_est[cur]))
        vS[i] = S_cur_corr if i == cur else _sim3_mul(Sic, S_cur_corr)
    eI, eJ, eS = [], [], []

    def add(i, j, Si, Sj):
        M = _sim3_mul(Sj, _sim3_inv(Si))
        if meas_noise:
            M = _sim3_mul(np.concatenate([_quat_from_rotvec(meas_noise * rng.normal(size=3)), meas_noise * rng.normal(size=3), [1.0]]), M)
        eI.append(i); eJ.append(j); eS.append(M)

    inserted = set()
    loop_side = [j for j in range(max(0, loop_kf - n_loop // 2), max(0, loop_kf - n_loop // 2) + n_loop) if j not in iso and j not in connected]
    if n_loop:
        for i in connected:
            for j in loop_side:
                if i == cur or j == loop_kf or (i + j) % 2 == 0:   # (the pair (cur, loop) always; the others by their weight)
                    add(i, j, vS[i], vS[j])
                    inserted.add((min(i, j), max(i, j)))
    old = []
    for _ in range(n_old_loops):
        i = int(rng.integers(n_kf // 2, n_kf)); j = int(rng.integers(0, max(1, n_kf // 4)))
        if i not in iso and j not in iso and i != j:
            old.append((i, j))
    parent = {}
    for i in range(n_kf):
        if i in iso:
            continue
        p = i - 1
        while p >= 0 and p in iso:
            p -= 1
        parent[i] = p
        if p >= 0:
            add(i, p, S_est[i], S_est[p])
        for (a, b) in old:
            if a == i and b < i:
                add(i, b, S_est[i], S_est[b])
        for j in range(i - 1, max(-1, i - band - 1), -1):
            if j in iso or j == p or (j, i) in inserted:
                continue
            add(i, j, S_est[i], S_est[j])
        if duplicate_every and p >= 0 and i % duplicate_every == 0:
            add(i, p, S_est[i], S_est[p])
    flags = np.zeros(n_kf, np.uint8)
    for f in fixed:
        flags[f] |= 1
    if fix_scale_on is not None:
        for f in fix_scale_on:
            flags[f] |= 2
    elif fix_scale:
        flags |= 2
    if fixed_pair_edge:
        fx = [f for f in fixed if f not in iso]
        if len(fx) >= 2:
            add(fx[1], fx[0], vS[fx[1]], _sim3_mul(np.concatenate([_quat_from_rotvec([0.01, 0.02, -0.01]), [fixed_pair_offset, 0.0, 0.02], [1.0]]), vS[fx[0]]))
    mpPos = np.zeros((n_points, 3), np.float32); mpRef = np.full(n_points, -1, np.int32)
    for m in range(n_points):
        r = int(rng.integers(0, n_kf))
        Swr = _sim3_inv(vS[r])
        Xc = np.array([rng.uniform(-2, 2), rng.uniform(-1, 1), rng.uniform(2, 8)])
        mpPos[m] = (Swr[7] * _quat_rot(Swr[:4], Xc) + Swr[4:7]).astype(np.float32)
        mpRef[m] = -1 if m % 10 == 9 else r
    return dict(kfSim3=vS, kfFlags=flags, eI=np.array(eI, np.int32), eJ=np.array(eJ, np.int32), eSji=np.array(eS, np.float64).reshape(-1, 8),
                mpPos=mpPos, mpRef=mpRef, cur=cur, loop=loop_kf, connected=connected, S_true=S_true)


# ---- the pose graph of map merging (Optimizer::OptimizeEssentialGraph, overload 2) ---------------------------------------------------------
def _pose7(S):
    """A Sim3 (qx qy qz qw tx ty tz s) as the float pose SE3(q, t / s)."""
    q = S[:4] / np.linalg.norm(S[:4])
    return np.concatenate([q, S[4:7] / S[7]]).astype(np.float32)


def _pose7_inv(p):
    p = p.astype(np.float64)
    qc = np.array([-p[0], -p[1], -p[2], p[3]])
    return np.concatenate([qc, -_quat_rot(qc, p[4:7])]).astype(np.float32)


def make_merge_graph_problem(n_fixed=6, n_window=5, n_nonfixed=20, overlap=True, band=3, n_old_loops=1, seed=0, n_points=0, fixed_links=True,
                             window_links=True, weld=True, reroot=True, corr_rot_deg=8.0, corr_trans=6.0, corr_scale=1.05, bad=(), isolated=(),
                             long_loop=False, drift_rot_deg=0.3, drift_scale=0.004, origin=(0.0, 0.0, 0.0)):
    """Two maps joined at a window, as LoopClosing::MergeLocal hands them to the second overload of Optimizer::OptimizeEssentialGraph
    (LoopClosing.cc:1747-1749), flattened for morb_optimize_essential_graph_merge.  Keyframes in ascending mnId: n_fixed keyframes of the
    merged map (vpFixedKFs, list bit 1), then the old map's n_nonfixed keyframes along a drifting chain (vpNonFixedKFs, bit 4).  The window
    (vpFixedCorrectedKFs, bit 2) is the last n_window keyframes of the chain with overlap (bits 2 | 4: vpLocalCurrentWindowKFs is a subset of
    vpCurrentMapKFs), or n_window further keyframes behind the chain without.  A window keyframe's mTcwBefMerge is its pose in the old map
    and its pose is that times the inverse of the merge's Sim3 correction (corr_*), as SE3 with t / s; every other keyframe's BefMerge
    members are Sophus' defaults.  `origin` moves the merged map's keyframes away from the world origin: an edge between two of them measures
    the parent's pose itself (the reference's identity Swi), so its error, a constant of chi2, grows with that distance.  Topology: a fixed keyframe's parent is the one before it and its covisibles (weight >= 100) are those
    at most `band` before (fixed_links); the same along the chain and the window (window_links: edges between two window keyframes), plus
    n_old_loops old loop edges inside the chain and, with long_loop, one from the last chain keyframe to the first; with reroot the window's
    spanning tree hangs from the merged map as MergeLocal leaves it — the newest window keyframe's parent is the last fixed keyframe, every
    other window keyframe's parent is the next one — and with weld each window keyframe is covisible with two fixed keyframes.  `bad`
    keyframes (indices before removal) are bad: no vertex, no edge, so a child of one has no spanning-tree edge; `isolated` non-fixed
    keyframes have a fixed keyframe as their only candidate, which the good / bad rule drops.  Candidates in the insertion order of
    Optimizer.cc:1888-1999: vpFixedKFs, vpFixedCorrectedKFs, vpNonFixedKFs, so an overlapped keyframe is visited twice; per keyframe the
    parent, the loop edges with a smaller id, the covisibles with a smaller id that are neither parent, child nor loop edge.  Points: n_points
    with references over every list, every eighth -1.  Returns a dict: kfLists, kfTcw, kfTwc, kfTcwBefMerge, kfTwcBefMerge, cI, cJ, mpPos,
    mpRef, plus window (vertices) and ids (vertex -> index before removal)."""
    rng = np.random.default_rng(seed)
    n_chain = n_nonfixed if overlap else n_nonfixed + n_window
    n_all = n_fixed + n_chain
    chain0 = n_fixed
    window = list(range(n_all - n_window, n_all))
    lists = np.zeros(n_all, np.uint8)
    lists[:n_fixed] = 1
    lists[chain0:chain0 + n_nonfixed] = 4
    for w in window:
        lists[w] |= 2
    # the old map: a camera on a circle looking along its tangent, with drift along the chain
    S_true = np.zeros((n_chain, 8))
    for i in range(n_chain):
        a = 2 * np.pi * i / max(n_chain, 8)
        q = _quat_from_rotvec(np.array([0.05 * np.sin(3 * a), -a, 0.03 * np.cos(2 * a)]))
        c = np.array([6 * np.cos(a), 0.2 * np.sin(5 * a), 6 * np.sin(a)])
        S_true[i] = np.concatenate([q, -_quat_rot(q, c), [1.0]])
    S_old = np.zeros_like(S_true)
    S_old[0] = S_true[0]
    for i in range(1, n_chain):
        rel = _sim3_mul(S_true[i], _sim3_inv(S_true[i - 1]))
        dq = _quat_from_rotvec(np.deg2rad(drift_rot_deg) * (np.array([0.2, 1.0, 0.1]) + 0.3 * rng.normal(size=3)))
        rel = np.concatenate([_quat_mul(dq, rel[:4]), (1.0 - drift_scale * (1 + 0.3 * rng.normal())) * _quat_rot(dq, rel[4:7]), [1.0]])
        S_old[i] = _sim3_mul(rel, S_old[i - 1])
        S_old[i, :4] /= np.linalg.norm(S_old[i, :4])
    # the merge's correction: Scw_corrected = Scw_old * G^-1
    gq = _quat_from_rotvec(np.deg2rad(corr_rot_deg) * np.array([0.3, 0.9, -0.2]) / np.linalg.norm([0.3, 0.9, -0.2]))
    G = np.concatenate([gq, corr_trans * np.array([0.5, -0.2, 0.8]), [corr_scale]])
    Ginv = _sim3_inv(G)
    ident = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
    Tcw, Twc = np.zeros((n_all, 7), np.float32), np.zeros((n_all, 7), np.float32)
    TcwBef, TwcBef = np.tile(ident, (n_all, 1)), np.tile(ident, (n_all, 1))
    for v in range(n_all):
        if v < n_fixed:   # the merged map: keyframes near where the correction puts the window
            a = 2 * np.pi * (n_chain - 1 - 0.7 * (n_fixed - v)) / max(n_chain, 8)
            q = _quat_from_rotvec(np.array([0.02, -a, 0.01]))
            c = np.array([6.3 * np.cos(a), 0.1, 6.3 * np.sin(a)]) + np.asarray(origin, np.float64)
            Tcw[v] = _pose7(_sim3_mul(np.concatenate([q, -_quat_rot(q, c), [1.0]]), Ginv))
        elif lists[v] & 2:
            TcwBef[v] = _pose7(S_old[v - chain0])
            TwcBef[v] = _pose7_inv(TcwBef[v])
            Tcw[v] = _pose7(_sim3_mul(S_old[v - chain0], Ginv))
        else:
            Tcw[v] = _pose7(S_old[v - chain0])
        Twc[v] = _pose7_inv(Tcw[v])
    # topology on the indices before removal
    dead, lone = set(int(b) for b in bad), set(int(i) for i in isolated)
    parent, covis, loops = {}, {v: [] for v in range(n_all)}, {v: set() for v in range(n_all)}
    for v in range(n_all):
        if v in lone:
            parent[v] = None
            covis[v] = [0]
            continue
        first = v == 0 or v == chain0
        in_window = v in window
        if not first and (fixed_links if v < n_fixed else True):
            p = v - 1
            while p in lone:
                p -= 1
            parent[v] = p if (p >= 0 and (p < n_fixed) == (v < n_fixed)) else None
        else:
            parent[v] = None
        if in_window and reroot and n_fixed:
            parent[v] = n_fixed - 1 if v == n_all - 1 else v + 1
        lo = 0 if v < n_fixed else chain0
        for j in range(v - 1, max(lo - 1, v - band - 1), -1):
            if j in lone or (v < n_fixed and not fixed_links):
                continue
            if in_window and j in window and not window_links:
                continue
            covis[v].append(j)
        if in_window and weld and n_fixed:
            covis[v] += [j for j in (n_fixed - 1, n_fixed - 2) if j >= 0]
    if not window_links:
        for w in window:
            if parent[w] in window:
                parent[w] = None
    olds = []
    for _ in range(n_old_loops):
        i = int(rng.integers(chain0 + n_nonfixed // 2, chain0 + n_nonfixed)); j = int(rng.integers(chain0, chain0 + max(1, n_nonfixed // 4)))
        if i not in lone and j not in lone and i != j and not (lists[i] & 2 and lists[j] & 2):
            olds.append((i, j))
    if long_loop:
        olds.append((chain0 + n_nonfixed - 1 - (n_window if overlap else 0), chain0))
    for i, j in olds:
        loops[i].add(j); loops[j].add(i)
    children = {v: set(c for c in range(n_all) if parent.get(c) == v) for v in range(n_all)}
    alive = [v for v in range(n_all) if v not in dead]
    row = {v: k for k, v in enumerate(alive)}
    cI, cJ = [], []
    order = [v for v in range(n_fixed)] + window + [v for v in range(chain0, chain0 + n_nonfixed)]
    for v in order:
        if v in dead:
            continue   # (a bad keyframe is neither good nor bad: every candidate of its own is dropped, :1907-1913)
        p = parent[v]
        if p is not None and p not in dead:
            cI.append(row[v]); cJ.append(row[p])
        for j in sorted(loops[v]):
            if j < v and j not in dead:
                cI.append(row[v]); cJ.append(row[j])
        for j in covis[v]:
            if j != p and j not in children[v] and j not in loops[v] and j not in dead and j < v:
                cI.append(row[v]); cJ.append(row[j])
    keep = np.array(alive, np.int64)
    lists, Tcw, Twc, TcwBef, TwcBef = lists[keep], Tcw[keep], Twc[keep], TcwBef[keep], TwcBef[keep]
    nKF = len(keep)
    mpPos = np.zeros((n_points, 3), np.float32); mpRef = np.full(n_points, -1, np.int32)
    for m in range(n_points):
        r = m % nKF if m < 2 * nKF else int(rng.integers(0, nKF))   # (every vertex, so every list, is somebody's reference)
        T = (TwcBef[r] if lists[r] & 2 else Twc[r]).astype(np.float64)
        Xc = np.array([rng.uniform(-2, 2), rng.uniform(-1, 1), rng.uniform(2, 8)])
        mpPos[m] = (_quat_rot(T[:4], Xc) + T[4:7]).astype(np.float32)
        mpRef[m] = -1 if m % 8 == 7 else r
    return dict(kfLists=lists, kfTcw=Tcw, kfTwc=Twc, kfTcwBefMerge=TcwBef, kfTwcBefMerge=TwcBef, cI=np.array(cI, np.int32), cJ=np.array(cJ, np.int32),
                mpPos=mpPos, mpRef=mpRef, window=[row[w] for w in window if w in row], ids=keep)


# ---- the 4-DoF pose graph of loop closing in an inertial map (Optimizer::OptimizeEssentialGraph4DoF) ---------------------------------------
def _rs_mul(a, b):
    """g2o::Sim3::operator* on (R, t, s)."""
    return a[0] @ b[0], a[2] * (a[0] @ b[1]) + a[1], a[2] * b[2]


def _rs_inv(a):
    return a[0].T, (-1.0 / a[2]) * (a[0].T @ a[1]), 1.0 / a[2]


def _quat_from_R_any(R):
    """Rotation matrix -> unit quaternion (x y z w) at any angle: the largest of the four candidates divides."""
    d = np.array([R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1], R[0, 0] + R[1, 1] + R[2, 2]])
    k = int(np.argmax(d))
    r = np.sqrt(1.0 + d[k])
    q = np.zeros(4)
    if k == 3:
        q[3] = 0.5 * r
        q[:3] = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (2 * r)
    else:
        i, j, l = k, (k + 1) % 3, (k + 2) % 3
        q[i] = 0.5 * r
        q[j] = (R[j, i] + R[i, j]) / (2 * r)
        q[l] = (R[l, i] + R[i, l]) / (2 * r)
        q[3] = (R[l, j] - R[j, l]) / (2 * r)
    return q / np.linalg.norm(q)


def make_pose_graph_4dof_problem(n_kf=30, band=3, n_loop=1, seed=0, n_old_loops=0, loop_kf=1, loop_yaw_deg=3.0, loop_trans=0.3, loop_scale=1.0,
                                 fixed=(0,), duplicate_every=0, fixed_pair_edge=False, isolated=(), n_points=0, drift_yaw_deg=0.3,
                                 drift_rp_deg=0.02, drift_trans=0.004, meas_noise=0.0, fixed_pair_offset=0.05):
    """A loop closure in an inertial map as LoopClosing::CorrectLoop hands it to Optimizer::OptimizeEssentialGraph4DoF, flattened for
    morb_optimize_essential_graph_4dof.  The world is gravity-aligned (z up).  Keyframes 0 .. n_kf-1 (ascending mnId): a body on a circle
    heading along its tangent, with a small true roll and pitch; the estimates drift per step in yaw (drift_yaw_deg), a little in roll and
    pitch (drift_rp_deg: what the IMU leaves) and in the length of the step (drift_trans).  A keyframe's pose and body state are what its
    float members hold, cast to double each on its own, so the two agree to float rounding only.  mPrevKF of keyframe i is the nearest
    earlier keyframe that is not `isolated`; covisibility (weight >= 100) joins keyframes at most `band` apart.  The current keyframe is
    the last one, the loop keyframe `loop_kf`.  The loop's correction is a yaw about the vertical and a translation of the world
    (loop_yaw_deg, loop_trans), with loop_scale in the corrected Sim3: CorrectedSim3 is propagated to the keyframes within `band` of the
    current one as LoopClosing.cc does, and their vertices are built from its inverse (ImuCamPose's third constructor, in double).
    Edges in the insertion order of Optimizer.cc:5236-5426 (vertex 0 = the later keyframe): the LoopConnections of the connected keyframes to
    the n_loop keyframes around the loop keyframe (measured between vScw), then per keyframe its mPrevKF link, its old loop edges
    (n_old_loops random long-range pairs), its covisibility edges and, every `duplicate_every`-th keyframe, a second edge on the mPrevKF
    pair; all measured between the non-corrected poses.  Each measurement is the rotation and the translation of the Sim3 product.
    fixed: fixed vertices; fixed_pair_edge adds an edge between two fixed vertices, its measurement off by fixed_pair_offset (a constant
    of chi2); `isolated` keyframes carry no edge.  Points: n_points with a reference keyframe each (every tenth -1).
    Returns a dict: kfPose, kfBody, kfFixed, Tcb12, eI, eJ, eTij, mpPos, mpRef, kfScw, plus cur, loop, connected."""
    rng = np.random.default_rng(seed)
    iso = set(int(i) for i in isolated)

    def rz(a):
        return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])

    Rcb = (np.array([[0, -1.0, 0], [0, 0, -1.0], [1.0, 0, 0]]) @ _rot_from_rotvec(np.array([0.01, -0.02, 0.015]))).astype(np.float32)
    tcb = np.array([0.05, -0.02, 0.01], np.float32)
    Tcb12 = np.concatenate([Rcb.ravel(), tcb]).astype(np.float32)
    Rcb_d, tcb_d = Rcb.astype(np.float64), tcb.astype(np.float64)
    # true body poses, then the drifted estimates
    Rt, pt = [], []
    for i in range(n_kf):
        a = 2 * np.pi * i / max(n_kf, 8)
        Rt.append(rz(a + np.pi / 2) @ _rot_from_rotvec(np.array([0.03 * np.sin(3 * a), 0.02 * np.cos(2 * a), 0.0])))
        pt.append(np.array([6 * np.cos(a), 6 * np.sin(a), 0.2 * np.sin(5 * a)]))
    Re, pe = [Rt[0]], [pt[0]]
    for i in range(1, n_kf):
        dRt, dpt = Rt[i - 1].T @ Rt[i], Rt[i - 1].T @ (pt[i] - pt[i - 1])
        dy = np.deg2rad(drift_yaw_deg) * (1 + 0.3 * rng.normal())
        drp = np.deg2rad(drift_rp_deg) * rng.normal(size=2)
        dRe = dRt @ rz(dy) @ _rot_from_rotvec(np.array([drp[0], drp[1], 0.0]))
        dpe = (1.0 - drift_trans * (1 + 0.3 * rng.normal())) * dpt
        Re.append(Re[i - 1] @ dRe); pe.append(pe[i - 1] + Re[i - 1] @ dpe)
    # the keyframes' float members, each cast to double on its own
    S_est, body = [], np.zeros((n_kf, 12))
    for i in range(n_kf):
        Rbw = Re[i].T
        Rcw = (Rcb_d @ Rbw).astype(np.float32).astype(np.float64)
        tcw = (Rcb_d @ (-Rbw @ pe[i]) + tcb_d).astype(np.float32).astype(np.float64)
        S_est.append((Rcw, tcw, 1.0))
        body[i, :9] = Re[i].astype(np.float32).astype(np.float64).ravel(); body[i, 9:] = pe[i].astype(np.float32).astype(np.float64)
    cur = n_kf - 1
    while cur in iso:
        cur -= 1
    connected = [i for i in range(max(0, cur - band), cur + 1) if i not in iso]
    # the loop's correction W of the world (a yaw and a translation): Twc <- W Twc, so Scw <- Scw W^-1; the corrected Sim3 carries loop_scale
    W = (rz(np.deg2rad(loop_yaw_deg)), loop_trans * np.array([0.8, -0.5, 0.1]), 1.0)
    cc = _rs_mul(S_est[cur], _rs_inv(W))
    S_cur_corr = (cc[0], loop_scale * cc[1], loop_scale)
    vS = list(S_est)   # vScw: CorrectedSim3's entry, or the pose
    pose = np.zeros((n_kf, 12))
    for i in range(n_kf):
        pose[i, :9] = S_est[i][0].ravel(); pose[i, 9:] = S_est[i][1]
    for i in connected:
        vS[i] = S_cur_corr if i == cur else _rs_mul(_rs_mul(S_est[i], _rs_inv(S_est[cur])), S_cur_corr)
        Rwc, twc, _ = _rs_inv(vS[i])   # VertexPose4DoF(Rwc, twc, pKF)
        body[i, :9] = (Rwc @ Rcb_d).ravel(); body[i, 9:] = Rwc @ tcb_d + twc
        pose[i, :9] = Rwc.T.ravel(); pose[i, 9:] = -Rwc.T @ twc
    eI, eJ, eT = [], [], []

    def add(i, j, Si, Sj):
        M = _rs_mul(Si, _rs_inv(Sj))
        if meas_noise:
            M = _rs_mul((_rot_from_rotvec(meas_noise * rng.normal(size=3)), meas_noise * rng.normal(size=3), 1.0), M)
        eI.append(i); eJ.append(j); eT.append(np.concatenate([M[0].ravel(), M[1]]))

    inserted = set()
    loop_side = [j for j in range(max(0, loop_kf - n_loop // 2), max(0, loop_kf - n_loop // 2) + n_loop) if j not in iso and j not in connected]
    if n_loop:
        for i in connected:
            for j in loop_side:
                if i == cur or j == loop_kf or (i + j) % 2 == 0:   # (the pair (cur, loop) always; the others by their weight)
                    add(i, j, vS[i], vS[j])
                    inserted.add((min(i, j), max(i, j)))
    old = []
    for _ in range(n_old_loops):
        i = int(rng.integers(n_kf // 2, n_kf)); j = int(rng.integers(0, max(1, n_kf // 4)))
        if i not in iso and j not in iso and i != j:
            old.append((i, j))
    for i in range(n_kf):
        if i in iso:
            continue
        p = i - 1
        while p >= 0 and p in iso:
            p -= 1
        if p >= 0:
            add(i, p, S_est[i], S_est[p])
        for (a, b) in old:
            if a == i and b < i:
                add(i, b, S_est[i], S_est[b])
        for j in range(i - 1, max(-1, i - band - 1), -1):
            if j in iso or j == p or (j, i) in inserted:
                continue
            add(i, j, S_est[i], S_est[j])
        if duplicate_every and p >= 0 and i % duplicate_every == 0:
            add(i, p, S_est[i], S_est[p])
    fx = np.zeros(n_kf, np.uint8)
    for f in fixed:
        fx[f] = 1
    if fixed_pair_edge:
        ff = [f for f in fixed if f not in iso]
        if len(ff) >= 2:
            add(ff[1], ff[0], vS[ff[1]], _rs_mul((_rot_from_rotvec(np.array([0.01, 0.02, -0.01])), np.array([fixed_pair_offset, 0.0, 0.02]), 1.0), vS[ff[0]]))
    scw = np.array([np.concatenate([_quat_from_R_any(S[0]), S[1], [S[2]]]) for S in vS])
    mpPos = np.zeros((n_points, 3), np.float32); mpRef = np.full(n_points, -1, np.int32)
    for m in range(n_points):
        r = int(rng.integers(0, n_kf))
        Swr = _rs_inv(vS[r])
        Xc = np.array([rng.uniform(-2, 2), rng.uniform(-1, 1), rng.uniform(2, 8)])
        mpPos[m] = (Swr[2] * (Swr[0] @ Xc) + Swr[1]).astype(np.float32)
        mpRef[m] = -1 if m % 10 == 9 else r
    return dict(kfPose=pose, kfBody=body, kfFixed=fx, Tcb12=Tcb12, eI=np.array(eI, np.int32), eJ=np.array(eJ, np.int32),
                eTij=np.array(eT, np.float64).reshape(-1, 12), mpPos=mpPos, mpRef=mpRef, kfScw=scw, cur=cur, loop=loop_kf, connected=connected)


# ---- loop closing's global bundle adjustment: Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust) ------------
def make_global_ba_problem(n_kf=40, reach=6, n_points=600, n_loop_points=0, seed=0, mono_frac=0.3, kb8=False, n_fixed=1, step=0.12,
                           kf_deg=0.3, kf_trans=0.02, point_noise=0.03, noise_px=1.0, right_frac=0.6, obs_frac=0.8, loop_span=3,
                           single_free_points=0, fixed_only_points=0, mono_single_points=0, idle_kf=None, idle_points=0, at_truth=False,
                           near_plane_point=False, cam=EUROC_CAM):
    """Input of the whole-map bundle adjustment: n_kf keyframes along a path, in ascending id (keyframes 0 .. n_fixed - 1 fixed: the map's
    initial keyframe, and what the caller fixes besides), looking sideways at n_points points.  Every point is seen by keyframes within
    `reach` of one another (a share obs_frac of that window, at least two), so the reduced system is a band of `reach` blocks;
    n_loop_points far points are seen from both ends of the path (its first and last loop_span keyframes) and give the long rows.  Poses,
    points and observations carry noise (kf_deg, kf_trans, point_noise, noise_px times the level's sigma).  mono_frac: the share of monocular
    observations on the pinhole camera (1.0: none stereo).  kb8: the TUM-VI KannalaBrandt8 rig, eObs is [nE, 2] and `rig` = dict(eRight, camL,
    camR, Trl): a left observation, and with probability right_frac the right camera's of the same keyframe behind it (a ToBody edge, the
    same (keyframe, point) pair).  Edges are ordered by point, then by keyframe, left before right.
    The named scenes: single_free_points points seen by ONE free keyframe only; fixed_only_points seen by fixed keyframes only;
    mono_single_points with one monocular observation; idle_kf: a free keyframe that observes nothing; idle_points: points nobody observes;
    at_truth: no noise anywhere (the first step is already too small to move chi2); near_plane_point: the last point lies 2e-38 in front of
    the focal plane of its first free observer, whose pose is the identity, and carries an information of 3e38 there: chi2 stays finite, the
    point's Hessian block does not survive its inversion, and every factorisation fails on a NaN pivot."""
    rng = np.random.default_rng(0x6BA00 + seed)
    Trl_m = np.linalg.inv(TUMVI_T_C1_C2)
    if at_truth:
        kf_deg = kf_trans = point_noise = noise_px = 0.0
    poses = []
    for i in range(n_kf):
        c = np.array([i * step, rng.normal(0, 0.03), rng.normal(0, 0.03)])
        q_wc = _quat_from_rotvec(rng.normal(0, 0.02, 3))
        q_cw = q_wc * np.array([-1, -1, -1, 1])
        poses.append(np.concatenate([q_cw, -_quat_rot(q_cw, c)]))
    poses = np.array(poses)
    free = [k for k in range(n_fixed, n_kf) if k != idle_kf]
    zr = (2.0, 8.0) if kb8 else (3.0, 10.0)
    X, seen_by = [], []

    def place(kfs, far=False):
        x0 = np.mean([k * step for k in kfs])
        z = rng.uniform(30, 40) if far else rng.uniform(*zr)
        X.append(np.array([x0 + rng.uniform(-1, 1) * (0.2 * z), rng.uniform(-0.25, 0.25) * z, z]))
        seen_by.append(sorted(int(k) for k in kfs))

    usable = [k for k in range(n_kf) if k != idle_kf]
    for j in range(n_points):
        k0 = int(rng.integers(0, max(n_kf - 1 - reach, 0) + 1))       # (reach >= n_kf - 1: every window is the whole path)
        window = [k for k in range(k0, min(k0 + reach + 1, n_kf)) if k != idle_kf]
        if len(window) < 2:
            window = usable[-2:]
        take = max(2, int(round(obs_frac * len(window))))
        place(rng.choice(window, size=min(take, len(window)), replace=False))
    for j in range(n_loop_points):
        ends = [k for k in list(range(min(loop_span, n_kf))) + list(range(max(n_kf - loop_span, 0), n_kf)) if k != idle_kf]
        place(sorted(set(ends)), far=True)
    single = []
    for j in range(single_free_points):
        single.append(len(X)); place([free[int(rng.integers(0, len(free)))]])
    for j in range(fixed_only_points):
        place(list(range(n_fixed)))
    mono_single = []
    for j in range(mono_single_points):
        mono_single.append(len(X)); place([free[int(rng.integers(0, len(free)))]])
    for j in range(idle_points):
        place([usable[0]]); seen_by[-1] = []
    X = np.array(X)
    eKF, eMP, eObs, eInv, eRight = [], [], [], [], []
    for j, kfs in enumerate(seen_by):
        for kf in kfs:
            Xc = _quat_rot(poses[kf][:4], X[j]) + poses[kf][4:]
            s = 1.2 ** int(rng.integers(0, 8))
            if kb8:
                for right in (0, 1):
                    if right and (rng.random() > right_frac or j in mono_single):
                        continue
                    Xs = Trl_m[:3, :3] @ Xc + Trl_m[:3, 3] if right else Xc
                    assert Xs[2] > 0.4
                    o = kb8_project(TUMVI_CAM_R if right else TUMVI_CAM_L, Xs[None])[0] + rng.normal(0, noise_px, 2) * s
                    eKF.append(kf); eMP.append(j); eObs.append(o); eInv.append(1.0 / s ** 2); eRight.append(right)
            else:
                assert Xc[2] > 0.5
                u = cam["fx"] * Xc[0] / Xc[2] + cam["cx"]; v = cam["fy"] * Xc[1] / Xc[2] + cam["cy"]
                o = np.array([u, v, u - cam["bf"] / Xc[2]]) + rng.normal(0, noise_px, 3) * s
                if rng.random() < mono_frac or j in mono_single or Xc[2] > 25.0:   # (a far point has no usable disparity)
                    o[2] = -1
                elif j in single:
                    o[2] = max(o[2], 0.0)
                o[2] = -1 if o[2] < 0 else o[2]
                eKF.append(kf); eMP.append(j); eObs.append(o); eInv.append(1.0 / s ** 2)
    pose0 = poses.copy()
    for i in range(n_fixed, n_kf):
        nq = _quat_from_rotvec(rng.normal(0, 1, 3) / np.sqrt(3) * np.deg2rad(kf_deg))
        pose0[i] = np.concatenate([_quat_mul(nq, poses[i][:4]), _quat_rot(nq, poses[i][4:]) + rng.normal(0, 1, 3) / np.sqrt(3) * kf_trans])
    X0 = X + rng.normal(0, point_noise, X.shape)
    eInv = np.array(eInv, np.float32)
    if near_plane_point:
        j = len(X) - 1 - idle_points
        e = next(k for k in range(len(eKF)) if eMP[k] == j and eKF[k] >= n_fixed)
        pose0[eKF[e]] = np.array([0, 0, 0, 1.0, 0, 0, 0])               # the identity exactly: the camera coordinates are the point's own
        X0[j] = np.array([0.5, 0.25, 2e-38])
        eInv[e] = 3e38
    fixed = np.zeros(n_kf, np.uint8); fixed[:n_fixed] = 1
    out = dict(kfPose=pose0.astype(np.float32), kfFixed=fixed, mpPos=X0.astype(np.float32), eKF=np.array(eKF, np.int32),
               eMP=np.array(eMP, np.int32), eInvSigma2=eInv, true_poses=poses, true_points=X, cam=cam, rig=None,
               single=np.array(single, np.int32), mono_single=np.array(mono_single, np.int32))
    if kb8:
        Trl7 = np.concatenate([_quat_from_R(Trl_m[:3, :3]), Trl_m[:3, 3]]).astype(np.float32)
        out.update(eObs=np.array(eObs, np.float32).reshape(-1, 2), rig=dict(eRight=np.array(eRight, np.uint8), camL=TUMVI_CAM_L, camR=TUMVI_CAM_R, Trl=Trl7))
    else:
        out["eObs"] = np.array(eObs, np.float32).reshape(-1, 3)
    return out


# ---- the inertial whole-map bundle adjustment (Optimizer::FullInertialBA) -----------------------------------------------------------------
def make_full_inertial_ba_problem(n_kf=40, reach=6, n_points=600, n_loop_points=0, seed=0, mono_frac=0.3, kb8=False, init=False, no_imu=(),
                                  n_fixed=0, observers=0, observer_frac=0.5, n_imu=20, step=0.12, kf_deg=0.3, kf_trans=0.02, vel_noise=0.03, bias_noise=1.0,
                                  point_noise=0.03, noise_px=1.0, right_frac=0.6, obs_frac=0.8, loop_span=3, idle_points=0, at_truth=False,
                                  near_plane_point=None, prior_g=1e2, prior_a=1e6, cam=EUROC_CAM):
    """Input of the inertial whole-map bundle adjustment (morb_full_inertial_ba): make_global_ba_problem's map — n_kf keyframes in ascending
    id along a path, every point seen by keyframes within `reach` of one another (a share obs_frac of that window), n_loop_points far points
    seen from both ends — with ONE temporal chain through all keyframes whose links carry n_imu IMU samples of a smooth motion, as
    make_inertial_ba_problem synthesises them.  Nothing is fixed unless asked: kfKind is 0 for every keyframe that enters a link.  no_imu:
    keyframes with !bImu, kind 3, which cut the chain on both sides (a keyframe left without any link is kind 3 too); n_fixed: the first
    n_fixed keyframes are fixed — kind 1 where they enter a link (n_fixed = 2 gives a link between two fixed keyframes), else kind 2;
    observers: extra fixed keyframes of kind 2 behind the chain, one of which sees a share observer_frac of the points.  init: bInit — `bias6` (gyro, accelerometer) is the shared bias the caller
    takes from the last keyframe, prior_g / prior_a the priors.  kb8: the TUM-VI rig, every observation monocular, eRight marks the right
    camera's (behind the left one of the same keyframe and point, with probability right_frac); eObs is [nE, 3] either way.  Edges are ordered
    by point, then keyframe, left before right.  idle_points: points nobody observes; at_truth: no noise anywhere; near_plane_point = k: the
    body-camera transform is the identity, keyframe k's pose too, and the last point lies 2e-38 in front of its focal plane with an
    information of 3e38 there (global BA's scene: the point's Hessian block does not survive its inversion)."""
    rng = np.random.default_rng(0xF1BA00 + seed)
    if at_truth:
        kf_deg = kf_trans = vel_noise = bias_noise = point_noise = noise_px = 0.0
    g = np.array([0, 0, -9.81])
    dt = 1.0 / IMU_FREQ
    bg = rng.normal(0, 0.01, 3); ba = rng.normal(0, 0.05, 3)
    Tbc = np.eye(4) if near_plane_point is not None else EUROC_TBC
    Rcb = Tbc[:3, :3].T; tcb = -Rcb @ Tbc[:3, 3]
    Trl = np.linalg.inv(TUMVI_T_C1_C2)
    # the body starts so that the camera's x axis is the direction of travel: the cameras look sideways at the points
    R = _rot_from_rotvec(rng.normal(0, 0.05, 3)); p = rng.normal(0, 0.1, 3)
    T = n_imu * dt
    v = R @ Tbc[:3, 0] * (step / T) + rng.normal(0, 0.02, 3)
    states = [(R, p, v)]
    acc, gyro, dts, start = [], [], [], [0]
    for k in range(n_kf - 1):
        w_b = rng.normal(0, 0.05, 3); a_w = rng.normal(0, 0.3, 3)
        for i in range(n_imu):
            Rm = R @ _rot_from_rotvec(w_b * (i + 0.5) * dt)
            acc.append(Rm.T @ (a_w - g) + ba + rng.normal(0, 0.02, 3))
            gyro.append(w_b + bg + rng.normal(0, 0.002, 3))
            dts.append(dt)
        R, p, v = R @ _rot_from_rotvec(w_b * T), p + v * T + 0.5 * a_w * T * T, v + a_w * T
        states.append((R, p, v))
        start.append(len(dts))
    for _ in range(observers):
        Rk, pk, _v = states[int(rng.integers(0, n_kf))]
        states.append((Rk @ _rot_from_rotvec(rng.normal(0, 0.03, 3)), pk + rng.normal(0, 0.1, 3), np.zeros(3)))
    nKF = len(states)
    # the chain: link k joins keyframes k and k + 1 unless one of them has no IMU
    cut = set(int(k) for k in no_imu)
    links = [k for k in range(n_kf - 1) if k not in cut and k + 1 not in cut]
    linked = set(links) | set(k + 1 for k in links)
    kind = np.array([(1 if k in linked else 2) if (k < n_fixed or k >= n_kf) else (0 if k in linked else 3) for k in range(nKF)], np.uint8)
    cams = [(Rcb @ Rk.T, Rcb @ (-Rk.T @ pk) + tcb) for Rk, pk, _ in states]
    zr = (2.0, 8.0) if kb8 else (3.0, 10.0)
    X, seen_by = [], []

    def place(kfs, far=False):
        Rm, tm = cams[sorted(kfs)[len(kfs) // 2]]
        z = rng.uniform(30, 40) if far else rng.uniform(*zr)
        xc = np.array([rng.uniform(-1, 1) * (0.2 * z), rng.uniform(-0.25, 0.25) * z, z])
        X.append(Rm.T @ (xc - tm))
        seen_by.append(sorted(int(k) for k in kfs))

    for j in range(n_points):
        k0 = int(rng.integers(0, max(n_kf - 1 - reach, 0) + 1))
        window = list(range(k0, min(k0 + reach + 1, n_kf)))
        take = max(2, int(round(obs_frac * len(window))))
        kfs = list(rng.choice(window, size=min(take, len(window)), replace=False))
        if observers and rng.random() < observer_frac:
            kfs.append(int(rng.integers(n_kf, nKF)))
        place(kfs)
    for j in range(n_loop_points):
        place(sorted(set(list(range(min(loop_span, n_kf))) + list(range(max(n_kf - loop_span, 0), n_kf)))), far=True)
    for j in range(idle_points):
        place([0]); seen_by[-1] = []
    X = np.array(X)
    w_img = 512 if kb8 else 752
    h_img = 512 if kb8 else 480
    eKF, eMP, eObs, eInv, eRight = [], [], [], [], []
    for j, kfs in enumerate(seen_by):
        for kf in kfs:
            Rcw, tcw = cams[kf]
            xc = Rcw @ X[j] + tcw
            s = 1.2 ** int(rng.integers(0, 8))
            if xc[2] < 0.5:
                continue
            if kb8:
                for right in (0, 1):
                    if right and rng.random() > right_frac:
                        continue
                    xs = Trl[:3, :3] @ xc + Trl[:3, 3] if right else xc
                    if xs[2] < 0.4:
                        continue
                    uv = kb8_project(TUMVI_CAM_R if right else TUMVI_CAM_L, xs[None])[0]
                    if not (5 < uv[0] < w_img - 5 and 5 < uv[1] < h_img - 5):
                        continue
                    o = uv + rng.normal(0, noise_px, 2) * s * 0.5
                    eKF.append(kf); eMP.append(j); eObs.append([o[0], o[1], -1.0]); eInv.append(4.0 / s ** 2); eRight.append(right)
            else:
                u = cam["fx"] * xc[0] / xc[2] + cam["cx"]; vv = cam["fy"] * xc[1] / xc[2] + cam["cy"]
                if not (0 <= u < w_img and 0 <= vv < h_img):
                    continue
                o = np.array([u, vv, u - cam["bf"] / xc[2]]) + rng.normal(0, noise_px, 3) * s
                if rng.random() < mono_frac or xc[2] > 25.0 or o[2] < 0:
                    o[2] = -1
                eKF.append(kf); eMP.append(j); eObs.append(o); eInv.append(1.0 / s ** 2); eRight.append(0)
    true = np.stack([np.concatenate([Rk.ravel(), pk, vk, bg, ba]) for Rk, pk, vk in states])
    init_s = true.copy()
    for k in range(nKF):
        if kind[k] in (1, 2):
            continue
        Rk, pk, vk = states[k]
        Rk = Rk @ _rot_from_rotvec(rng.normal(0, 1, 3) / np.sqrt(3) * np.deg2rad(kf_deg))
        init_s[k, :9] = Rk.ravel(); init_s[k, 9:12] = pk + rng.normal(0, 1, 3) / np.sqrt(3) * kf_trans
        if kind[k] == 0:
            init_s[k, 12:15] = vk + rng.normal(0, vel_noise, 3)
            init_s[k, 15:18] += rng.normal(0, 0.001, 3) * bias_noise; init_s[k, 18:21] += rng.normal(0, 0.005, 3) * bias_noise
    bias6 = np.concatenate([bg + rng.normal(0, 0.001, 3) * bias_noise, ba + rng.normal(0, 0.005, 3) * bias_noise])
    X0 = X + rng.normal(0, point_noise, X.shape)
    eInv = np.array(eInv, np.float32)
    eKF = np.array(eKF, np.int32); eMP = np.array(eMP, np.int32)
    if near_plane_point is not None:
        k = int(near_plane_point)
        j = len(X) - 1 - idle_points
        e = np.flatnonzero((eMP == j) & (eKF == k))
        assert len(e), "the last point is not seen by the near-plane keyframe"
        init_s[k, :9] = np.eye(3).ravel(); init_s[k, 9:12] = 0.0          # the identity exactly: the camera coordinates are the point's own
        X0[j] = np.array([0.5, 0.25, 2e-38])
        eInv[e[0]] = 3e38
    return dict(kfState=init_s.astype(np.float32), kfKind=kind, mpPos=X0.astype(np.float32), eKF=eKF, eMP=eMP,
                eObs=np.array(eObs, np.float32).reshape(-1, 3), eInvSigma2=eInv, eRight=np.array(eRight, np.uint8),
                iKF1=np.array(links, np.int32), iKF2=np.array(links, np.int32) + 1,
                imuStart=np.array(start, np.int32), acc=np.array(acc, np.float32), gyro=np.array(gyro, np.float32), dt=np.array(dts, np.float32),
                bias=np.concatenate([ba, bg]).astype(np.float32), Tbc12=np.concatenate([Tbc[:3, :3].ravel(), Tbc[:3, 3]]).astype(np.float32),
                cam=cam, rig28=tumvi_rig28() if kb8 else None, init=bool(init), bias6=bias6.astype(np.float32), priorG=float(prior_g),
                priorA=float(prior_a), true=true, truePts=X)


# ---- the map graph of Tracking::UpdateLocalMap (morb_update_local_map_batch) ------------------------------------------------------
def local_map_scene_from_rows(rows, nmp, kf_cap, frames, cap=None, order=None, bad_kf=(), bad_mp=(), covis=None, ncovis=10, parent=None,
                              prev=None, last_kf=None, extra_obs=(), seed=0):
    """The device tables of morb_update_local_map_batch from explicit keyframe rows.  rows: one sequence of map-point rows per keyframe
    (-1 = NULL, repeats allowed); the observations are derived from them (a point is observed by exactly the keyframes that hold it),
    plus extra_obs = (point, keyframe) pairs that deliberately break that.  frames: one sequence of map-point rows per query.  order:
    d_kfOrder or None (row order).  covis: per-keyframe neighbour lists, None = by shared points (descending, ties by row).  parent:
    array or None = the earlier keyframe sharing most points (keyframe 0 is the root).  prev: mPrevKF, None = row - 1.  last_kf: per
    query, None = -1.  Children are listed in `order` order, as a std::set<KeyFrame*> iterates.  Returns a dict of host arrays:
    kfMp i32 [nkf, kf_cap], kfCount, kfFlags u8, kfOrder (or None), covis i32 [nkf, ncovis], childStart / child, parent, prevKf,
    mpObsStart / mpObsKf, mpFlags u8, frameMp i32 [nq, cap], count, lastKf, the per-point arrays the gather reads (mpPw, mpNormal f32
    [nmp, 3], mpMaxD, mpMinD f32, mpDesc u8 [nmp, 32], mpIsBad, mpObserved u8) and the sizes nkf, nmp, kf_cap, cap, ncovis."""
    rng = np.random.default_rng(0x10ca1 + seed)
    nkf, nq = len(rows), len(frames)
    kfMp, kfCount = np.full((nkf, kf_cap), -1, np.int32), np.zeros(nkf, np.int32)
    for k, r in enumerate(rows):
        r = np.asarray(r, np.int32)
        assert len(r) <= kf_cap
        kfMp[k, :len(r)], kfCount[k] = r, len(r)
    held = (kfMp >= 0) & (np.arange(kf_cap)[None, :] < kfCount[:, None])
    codes = kfMp[held].astype(np.int64) * max(nkf, 1) + np.nonzero(held)[0]
    codes = np.unique(np.concatenate([codes, np.array([int(m) * max(nkf, 1) + int(k) for m, k in extra_obs], np.int64)]))   # (point, keyframe), sorted
    pm = np.stack([codes // max(nkf, 1), codes % max(nkf, 1)], 1)
    mpObsStart = np.zeros(nmp + 1, np.int32)
    np.add.at(mpObsStart, pm[:, 0] + 1, 1)
    mpObsStart = np.cumsum(mpObsStart).astype(np.int32)
    mpObsKf = pm[:, 1].astype(np.int32)
    kfFlags, mpFlags = np.zeros(nkf, np.uint8), np.zeros(nmp, np.uint8)
    kfFlags[list(bad_kf)] = 1
    mpFlags[list(bad_mp)] = 1
    order = None if order is None else np.asarray(order, np.int32)
    pos = np.arange(nkf) if order is None else order
    shared = None
    if covis is None or parent is None:
        step = max(nmp // 4096, 1)               # a sample of the points is enough to rank neighbours
        M = np.zeros((nkf, nmp // step + 1), np.float32)
        for k in range(nkf):
            r = kfMp[k, :kfCount[k]]
            r = r[(r >= 0) & (r % step == 0)]
            M[k, r // step] = 1
        shared = M @ M.T
        np.fill_diagonal(shared, 0)
    cv = np.full((nkf, max(ncovis, 1)), -1, np.int32)[:, :ncovis]
    for k in range(nkf):
        if covis is not None:
            nb = list(covis[k]) if k < len(covis) else []
        else:
            cand = np.flatnonzero(shared[k] > 0)
            nb = cand[np.lexsort((cand, -shared[k, cand]))][:ncovis]
        cv[k, :len(nb)] = nb[:ncovis]
    if parent is None:
        parent = np.full(nkf, -1, np.int32)
        for k in range(1, nkf):
            parent[k] = int(np.argmax(shared[k, :k])) if shared[k, :k].max() > 0 else k - 1
    parent = np.asarray(parent, np.int32)
    kids = [[] for _ in range(nkf)]
    for k in sorted(range(nkf), key=lambda k: pos[k]):
        if parent[k] >= 0:
            kids[parent[k]].append(k)
    childStart = np.concatenate([[0], np.cumsum([len(c) for c in kids])]).astype(np.int32)
    child = np.array([c for cs in kids for c in cs], np.int32)
    prevKf = np.arange(-1, nkf - 1, dtype=np.int32) if prev is None else np.asarray(prev, np.int32)
    cap = cap or max([len(f) for f in frames] + [1])
    frameMp, count = np.full((nq, cap), -1, np.int32), np.zeros(nq, np.int32)
    for q, f in enumerate(frames):
        frameMp[q, :len(f)], count[q] = np.asarray(f, np.int32), len(f)
    lastKf = np.full(nq, -1, np.int32) if last_kf is None else np.asarray(last_kf, np.int32)
    Pw = rng.normal(0, 3, (nmp, 3)).astype(np.float32)
    nrm = rng.normal(0, 1, (nmp, 3))
    maxD = rng.uniform(2, 20, nmp).astype(np.float32)
    return dict(kfMp=kfMp, kfCount=kfCount, kfFlags=kfFlags, kfOrder=order, covis=np.ascontiguousarray(cv), childStart=childStart, child=child,
                parent=parent, prevKf=prevKf, mpObsStart=mpObsStart, mpObsKf=mpObsKf, mpFlags=mpFlags, frameMp=frameMp, count=count,
                lastKf=lastKf, mpPw=Pw, mpNormal=(nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32), mpMaxD=maxD,
                mpMinD=(maxD / np.float32(3.58)).astype(np.float32), mpDesc=rng.integers(0, 256, (nmp, 32), dtype=np.uint8),
                mpIsBad=(mpFlags & 1).astype(np.uint8), mpObserved=(np.diff(mpObsStart) > 0).astype(np.uint8),
                nkf=nkf, nmp=nmp, kf_cap=kf_cap, cap=cap, ncovis=ncovis)


def make_local_map_scene(seed=0, nkf=60, nmp=2000, kf_cap=128, nq=4, cap=None, track=6, ncovis=10, shuffle_order=True, bad_kf_frac=0.05,
                         bad_mp_frac=0.03, null_frac=0.1, dup_frac=0.02, stray_frac=0.05):
    """A consistent synthetic map for Tracking::UpdateLocalMap: nkf keyframes along a trajectory, nmp points, point j seen by (most
    of) the keyframes of an interval of about `track` keyframes around its place, so that a frame at keyframe c is voted for by about
    2 track keyframes.  A keyframe's row holds its points in a shuffled feature order with null_frac NULL entries and dup_frac of
    them repeated once more (at most kf_cap entries: surplus observations are dropped on both sides).  The covisibility rows rank
    the keyframes by shared points, the spanning tree hangs every keyframe under the earlier one it shares most with, mPrevKF is the
    keyframe before, d_kfOrder a random permutation (shuffle_order), bad_kf_frac / bad_mp_frac of the rows are bad.  The nq query
    frames stand at keyframes spread over the trajectory: each holds most points of its keyframe and of the next one, stray_frac
    points from anywhere in the map (usually outside the local map) and NULLs; lastKf is its keyframe.  Returns
    local_map_scene_from_rows's dict."""
    rng = np.random.default_rng(0x5ce9e + seed)
    start = rng.integers(-track, nkf, nmp)
    length = rng.integers(2, 2 * track + 1, nmp)
    mp = np.repeat(np.arange(nmp), length)
    kf = np.concatenate([np.arange(s, s + n) for s, n in zip(start, length)]) if nmp else np.zeros(0, np.int64)
    keep = (kf >= 0) & (kf < nkf) & (rng.random(len(kf)) < 0.9)
    mp, kf = mp[keep], kf[keep]
    by_kf = np.argsort(kf, kind="stable")
    bounds = np.searchsorted(kf[by_kf], np.arange(nkf + 1))
    rows = []
    for k in range(nkf):
        r = rng.permutation(mp[by_kf[bounds[k]:bounds[k + 1]]])
        room = int(kf_cap / (1 + null_frac + dup_frac)) - 1
        r = r[:max(room, 0)]
        extra = [np.full(int(round(len(r) * null_frac)), -1, np.int64), r[:int(np.ceil(len(r) * dup_frac))]]
        r = np.concatenate([r] + extra)
        tail = rng.permutation(len(r))            # NULLs and repeats anywhere in the row
        rows.append(r[tail][:kf_cap])
    bad_kf = rng.choice(nkf, int(round(nkf * bad_kf_frac)), replace=False) if nkf else []
    bad_mp = rng.choice(nmp, int(round(nmp * bad_mp_frac)), replace=False) if nmp else []
    cap = cap or kf_cap
    frames, last = [], []
    for q in range(nq):
        c = int((q + 0.5) * nkf / max(nq, 1)) if nkf else -1
        pts = np.unique(np.concatenate([r[r >= 0] for r in rows[c:c + 2]])) if nkf else np.zeros(0, np.int64)
        pts = rng.permutation(pts)[:int(cap * 0.8)]
        f = np.concatenate([pts, rng.integers(0, max(nmp, 1), int(cap * stray_frac)) if nmp else [], np.full(int(cap * 0.1), -1)]).astype(np.int64)
        frames.append(rng.permutation(f)[:cap])
        last.append(c)
    order = rng.permutation(nkf) if shuffle_order else None
    return local_map_scene_from_rows(rows, nmp, kf_cap, frames, cap=cap, order=order, bad_kf=bad_kf, bad_mp=bad_mp, ncovis=ncovis,
                                     last_kf=last, seed=seed)
