"""Optimizer — host-side mirror of the reference's static Optimizer functions on the hot path
(include/Optimizer.h:46-139): PoseOptimization, LocalBundleAdjustment and the inertial functions of SURVEY 8(f) N1
(IMU preintegration, PoseInertialOptimizationLastKeyFrame / LastFrame, LocalInertialBA, InertialOptimization), over the device-resident kernels."""
import ctypes as C

import numpy as np

from .capi import HEADER, check, lib, ptr, stream_arg


# morb_imu_preintegrated (include/morb_hip.h) as a float32 record: field -> (offset, length), both in floats
_PREINT = HEADER.records["morb_imu_preintegrated"]
assert all(_PREINT[n].base == np.float32 for n in _PREINT.names)
PREINT_FIELDS = {n: (_PREINT.fields[n][1] // 4, int(np.prod(_PREINT[n].shape, dtype=int))) for n in _PREINT.names}
PREINT_FLOATS = _PREINT.itemsize // 4
# morb_sim3_solver_params / _state and morb_mlpnp_solver_params / _state as numpy records
SIM3_SOLVER_PARAMS, SIM3_SOLVER_STATE, MLPNP_SOLVER_PARAMS, MLPNP_SOLVER_STATE = (
    HEADER.records[f"morb_{s}_solver_{r}"] for s in ("sim3", "mlpnp") for r in ("params", "state"))
# the rows morb_two_view_reconstruction_batch writes to d_stats / d_fstats, index by index: the enums TwoViewStat / TwoViewFStat of
# include/morb/two_view_math.h (tests/test_two_view_cpu.py compares these tuples with what the compiler makes of the enums)
TWO_VIEW_STATS = ("N", "MODEL", "BEST_IT_H", "BEST_IT_F", "NINLIERS", "NHYP", "CHOSEN", "FAIL") + tuple(f"NGOOD{k}" for k in range(8))
TWO_VIEW_FSTATS = ("SH", "SF", "RH") + tuple(f"H21_{k}" for k in range(9)) + tuple(f"F21_{k}" for k in range(9)) + \
    tuple(f"PARALLAX{k}" for k in range(8))
TWO_VIEW_FAIL = ("NONE", "FEW_MATCHES", "ZERO_SCORE", "DEGENERATE_H", "AMBIGUOUS", "PARALLAX")
# d_status of morb_create_initial_map_monocular_batch (InitialMapStatus of include/morb/initial_map_math.h): the reset reasons are bits
INITIAL_MAP_STATUS = {"NOT_RUN": 0, "OK": 1, "RESET_MEDIAN": 2, "RESET_COUNT": 4}


class Optimizer:
    def __init__(self, device=0):
        self._L = lib()
        self._h = C.c_void_p()
        check(self._L.morb_optimizer_create(C.byref(self._h), device))
        self.device = device

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.morb_optimizer_destroy(self._h)
            self._h = None

    __del__ = close

    def set_exact_order(self, on=True):
        """PoseOptimization sums in edge order (the default: g2o's LM path decision for decision) or as a tree (~3 % faster, the trial count may differ by one); morb_optimizer_set_exact_order."""
        check(self._L.morb_optimizer_set_exact_order(self._h, 1 if on else 0))

    def info(self):
        """morb_optimizer_info: {"exact_order": 0|1, "mfma_chain": 0|1, "mfma_selftest": 1 passed | 0 device rejected | -1 not run} — which
        PoseOptimization path this handle runs."""
        a, b, c = C.c_int(-9), C.c_int(-9), C.c_int(-9)
        check(self._L.morb_optimizer_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"mfma_chain": a.value, "exact_order": b.value, "mfma_selftest": c.value}

    def PoseOptimization(self, hasMP, obs, invSigma2, Xw, pose, cam, count=None, out=None, stream=None):
        """Batched PoseOptimization.  Device tensors: hasMP u8 [F, cap], obs f32 [F, cap, 3] (x, y, uRight),
        invSigma2 f32 [F, cap], Xw f32 [F, cap, 3], pose f32 [F, 7] (in/out), count i32 [F] or None.
        Returns (nInliers i32 [F], outlier u8 [F, cap], stats i32 [F, 2]); pose is updated in place."""
        import torch
        F, cap = hasMP.shape
        if out is None:
            out = (torch.empty((F,), dtype=torch.int32, device=hasMP.device),
                   torch.zeros((F, cap), dtype=torch.uint8, device=hasMP.device),
                   torch.empty((F, 2), dtype=torch.int32, device=hasMP.device))
        st = stream_arg(stream)
        check(self._L.morb_pose_optimization_batch(self._h, F, cap, ptr(count), ptr(hasMP), ptr(obs), ptr(invSigma2), ptr(Xw),
                                                   cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["bf"], ptr(pose),
                                                   ptr(out[1]), ptr(out[0]), ptr(out[2]), st))
        return out

    def PoseOptimizationFisheye(self, hasMP, obs, invSigma2, Xw, pose, nLeft, count, camL, camR, Trl, out=None, stream=None):
        """PoseOptimization for a fisheye rig: features [0, nLeft[f]) left camera, the rest right camera ("ToBody").
        camL/camR: 8 floats; Trl: 7 floats (quaternion xyzw + translation, left-camera -> right-camera frame)."""
        import torch
        F, cap = hasMP.shape
        if out is None:
            out = (torch.empty((F,), dtype=torch.int32, device=hasMP.device),
                   torch.zeros((F, cap), dtype=torch.uint8, device=hasMP.device),
                   torch.empty((F, 2), dtype=torch.int32, device=hasMP.device))
        a = [np.ascontiguousarray(x, np.float32) for x in (camL, camR, Trl)]
        st = stream_arg(stream)
        check(self._L.morb_pose_optimization_fisheye_batch(self._h, F, cap, ptr(count), ptr(nLeft), ptr(hasMP), ptr(obs), ptr(invSigma2),
                                                           ptr(Xw), ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(pose), ptr(out[1]), ptr(out[0]),
                                                           ptr(out[2]), st))
        return out

    def OptimizeSim3(self, entry, Xw1, Xw2, i2, obs1, invSigma2_1, obs2, invSigma2_2, T1w, T2w, cam1, cam2, th2, fixScale, S12,
                     bAllPoints=False, count=None, out=None, stream=None):
        """Batched Optimizer::OptimizeSim3 (morb_optimize_sim3_batch).  Device tensors, P problems of up to cap KF1 features:
        entry u8 [P, cap] (bit 0 vpMatches1[i] != NULL, bit 1 pMP1 present, bit 2 pMP1 bad, bit 3 pMP2 bad), Xw1 / Xw2 f32 [P, cap, 3],
        i2 i32 [P, cap], obs1 / obs2 f32 [P, cap, 2], invSigma2_1 / invSigma2_2 f32 [P, cap], T1w / T2w f32 [P, 12] (R row-major + t),
        cam1 / cam2 f32 [P, 9] (kind 0 pinhole / 1 KB8 + 8 parameters), th2 f32 [P], fixScale u8 [P], S12 f64 [P, 8]
        (qx qy qz qw tx ty tz s; in / out, written only where the function reaches its end), count i32 [P] or None.  bAllPoints defaults
        to False as in the reference's declaration; invSigma2_2 of an i2 < 0 entry is mvInvLevelSigma2[0] (see include/morb_hip.h).
        Returns (nIn i32 [P], keep u8 [P, cap], stats i32 [P, 8]); keep[p, i] = vpMatches1[i] != NULL on return; stats = LM iterations
        and trials of phase 1, of phase 2, reached-the-end flag, correspondences, phase-1 outliers, nIn."""
        import torch
        P, cap = entry.shape
        if out is None:
            out = (torch.empty((P,), dtype=torch.int32, device=entry.device),
                   torch.empty((P, cap), dtype=torch.uint8, device=entry.device),
                   torch.empty((P, 8), dtype=torch.int32, device=entry.device))
        st = stream_arg(stream)
        check(self._L.morb_optimize_sim3_batch(self._h, P, cap, ptr(count), ptr(entry), ptr(Xw1), ptr(Xw2), ptr(i2), ptr(obs1), ptr(invSigma2_1),
                                               ptr(obs2), ptr(invSigma2_2), ptr(T1w), ptr(T2w), ptr(cam1), ptr(cam2), ptr(th2), ptr(fixScale),
                                               int(bool(bAllPoints)), ptr(S12), ptr(out[1]), ptr(out[0]), ptr(out[2]), st))
        return out

    def Sim3Solver(self, params, entry, Xw1, Xw2, sigma2_1, sigma2_2, rand, state, nIterations, inliers=None, hypInliers=None,
                   stream=None):
        """Batched Sim3Solver (morb_sim3_solver_batch): the constructor, SetRansacParameters and iterate(nIterations, ...) from
        state.iterations on.  Device tensors, P problems of up to cap KF1 features: params u8 [P, 192] (SIM3_SOLVER_PARAMS records),
        entry u8 [P, cap] (bits 0-5: matched, pMP1 present, pMP1 bad, pMP2 bad, indexKF1 < 0, indexKF2 < 0), Xw1 / Xw2 f32 [P, cap, 3],
        sigma2_1 / sigma2_2 f32 [P, cap] (mvLevelSigma2 of the two keypoints' octaves), rand i32 [P, randCap] (rand() values, three
        per iteration by global iteration number), state u8 [P, 212] (SIM3_SOLVER_STATE records, in / out; zero before the first
        call).  hypInliers i32 [P, hypCap] or None receives the inlier count of every iteration evaluated.  Returns
        (state, inliers u8 [P, cap], hypInliers); inliers = vbInliers, set only on convergence."""
        import torch
        P, cap = entry.shape
        if inliers is None:
            inliers = torch.empty((P, cap), dtype=torch.uint8, device=entry.device)
        hypCap = 0 if hypInliers is None else hypInliers.shape[1]
        st = stream_arg(stream)
        check(self._L.morb_sim3_solver_batch(self._h, P, cap, ptr(params), ptr(entry), ptr(Xw1), ptr(Xw2), ptr(sigma2_1), ptr(sigma2_2),
                                             int(nIterations), ptr(rand), rand.shape[1], ptr(state), ptr(inliers), ptr(hypInliers), hypCap,
                                             st))
        return state, inliers, hypInliers

    @staticmethod
    def sim3_solver_state(state):
        """The state tensor u8 [P, 212] -> numpy SIM3_SOLVER_STATE records [P]."""
        return np.frombuffer(state.cpu().numpy().tobytes(), SIM3_SOLVER_STATE).copy()

    def MLPnPsolver(self, params, entry, uv, sigma2, Xw, rand, state, bestInliers, nIterations, inliers=None, hypInliers=None, stream=None):
        """Batched MLPnPsolver (morb_mlpnp_solver_batch): the constructor, SetRansacParameters and iterate(nIterations, ...) from
        state.iterations on.  Device tensors, P problems of up to cap features: params u8 [P, 72] (MLPNP_SOLVER_PARAMS records), entry
        u8 [P, cap] (bit 0 matched, bit 1 bad map point, bit 2 feature index beyond mvKeysUn), uv f32 [P, cap, 2] (mvKeysUn[i].pt),
        sigma2 f32 [P, cap], Xw f32 [P, cap, 3], rand i32 [P, randCap] (rand() values, minSet per iteration by global iteration
        number), state u8 [P, 168] (MLPNP_SOLVER_STATE records, in / out; zero before the first call), bestInliers u8 [P, cap]
        (mvbBestInliers, in / out).  hypInliers i32 [P, hypCap] or None receives the inlier count of every iteration evaluated.
        Returns (state, inliers u8 [P, cap], hypInliers); inliers = vbInliers, set only when state.ok."""
        import torch
        P, cap = entry.shape
        if inliers is None:
            inliers = torch.empty((P, cap), dtype=torch.uint8, device=entry.device)
        hypCap = 0 if hypInliers is None else hypInliers.shape[1]
        st = stream_arg(stream)
        check(self._L.morb_mlpnp_solver_batch(self._h, P, cap, ptr(params), ptr(entry), ptr(uv), ptr(sigma2), ptr(Xw), int(nIterations),
                                              ptr(rand), rand.shape[1], ptr(state), ptr(bestInliers), ptr(inliers), ptr(hypInliers), hypCap,
                                              st))
        return state, inliers, hypInliers

    @staticmethod
    def mlpnp_solver_state(state):
        """The state tensor u8 [P, 168] -> numpy MLPNP_SOLVER_STATE records [P]."""
        return np.frombuffer(state.cpu().numpy().tobytes(), MLPNP_SOLVER_STATE).copy()

    def TwoViewReconstruction(self, img1, img2, count, kps, matches12, K4, sigma, rand, maxIterations=200, out=None, masks=False,
                              hypScores=False, stream=None):
        """Batched TwoViewReconstruction::Reconstruct (morb_two_view_reconstruction_batch), what Pinhole::ReconstructWithTwoViews runs
        for the monocular initialisation.  Device tensors, P problems over a keypoint pool: img1 / img2 i32 [P] (pool images), count
        i32 [nimg], kps [nimg, cap] KP_DTYPE records (mvKeysUn; a u8 view [nimg, cap, 28] will do), matches12 i32 [P, cap] (vnMatches12
        as SearchForInitialization writes it), K4 f32 [P, 4] (fx fy cx cy), sigma f32 [P], rand i32 [P, randCap >= 8 maxIterations]
        (rand() values, eight per iteration).  out = (ok i32 [P], T21 f32 [P, 12], P3D f32 [P, cap, 3], triangulated u8 [P, cap],
        stats i32 [P, len(TWO_VIEW_STATS)], fstats f32 [P, len(TWO_VIEW_FSTATS)]) or None.  masks / hypScores: True allocates, a tuple
        (inliersH, inliersF) u8 [P, cap] / a tensor f32 [P, 2, maxIterations] is used as given.  Returns a dict of all of them."""
        import torch
        P, cap = matches12.shape
        dev = matches12.device
        if out is None:
            out = (torch.empty((P,), dtype=torch.int32, device=dev), torch.empty((P, 12), dtype=torch.float32, device=dev),
                   torch.empty((P, cap, 3), dtype=torch.float32, device=dev), torch.empty((P, cap), dtype=torch.uint8, device=dev),
                   torch.empty((P, len(TWO_VIEW_STATS)), dtype=torch.int32, device=dev),
                   torch.empty((P, len(TWO_VIEW_FSTATS)), dtype=torch.float32, device=dev))
        if masks is True:
            masks = (torch.empty((P, cap), dtype=torch.uint8, device=dev), torch.empty((P, cap), dtype=torch.uint8, device=dev))
        if hypScores is True:
            hypScores = torch.empty((P, 2, max(int(maxIterations), 1)), dtype=torch.float32, device=dev)
        inlH, inlF = masks if masks else (None, None)
        hyp = hypScores if hypScores is not False else None
        st = stream_arg(stream)
        check(self._L.morb_two_view_reconstruction_batch(self._h, P, cap, ptr(img1), ptr(img2), ptr(count), ptr(kps), ptr(matches12), ptr(K4),
                                                         ptr(sigma), int(maxIterations), ptr(rand), rand.shape[1], ptr(out[0]), ptr(out[1]),
                                                         ptr(out[2]), ptr(out[3]), ptr(out[4]), ptr(out[5]), ptr(inlH), ptr(inlF), ptr(hyp),
                                                         st))
        return dict(ok=out[0], T21=out[1], P3D=out[2], triangulated=out[3], stats=out[4], fstats=out[5], inliersH=inlH, inliersF=inlF,
                    hypScores=hyp)

    def CreateInitialMapMonocular(self, params, img1, img2, count, kps, matches12, ok, T21, P3D, triangulated, nIterations=20, robust=True,
                                  depthScale=1.0, minTracked=50, cam8=None, kb8=False, stop=None, out=None, stream=None):
        """The numeric rest of Tracking::CreateInitialMapMonocular behind TwoViewReconstruction (morb_create_initial_map_monocular_batch):
        GlobalBundleAdjustemnt over the two keyframes and their points, the median depth of keyframe 1, the reset test, the rescaling
        and UpdateNormalAndDepth.  Device tensors, P problems over a keypoint pool: params = FrameParams (mvLevelSigma2, mvScaleFactors,
        the pinhole camera), img1 / img2 i32 [P], count i32 [nimg], kps [nimg, cap] KP_DTYPE records (mvKeysUn), matches12 i32 [P, cap],
        and what TwoViewReconstruction returned: ok i32 [P], T21 f32 [P, 12], P3D f32 [P, cap, 3], triangulated u8 [P, cap].  cam8 (host,
        8 floats) replaces the camera of params; kb8 selects KannalaBrandt8.  stop u8 [P] on the device or None.  depthScale: 1, 4 for
        IMU-monocular, 0 = no scaling.  Returns a dict: status i32 [P] (INITIAL_MAP_STATUS), Tcw2 f32 [P, 12], mpPos / mpNormal f32
        [P, cap, 3], mpDist f32 [P, cap, 2], hasMP u8 [P, cap], stats i32 [P, 4] (points, outer iterations, trials, stop seen), chi2 f64
        [P, 2], median f32 [P]."""
        import torch
        P, cap = matches12.shape
        dev = matches12.device
        if out is None:
            f32, i32 = torch.float32, torch.int32
            out = dict(status=torch.zeros((P,), dtype=i32, device=dev), Tcw2=torch.zeros((P, 12), dtype=f32, device=dev),
                       mpPos=torch.zeros((P, cap, 3), dtype=f32, device=dev), mpNormal=torch.zeros((P, cap, 3), dtype=f32, device=dev),
                       mpDist=torch.zeros((P, cap, 2), dtype=f32, device=dev), hasMP=torch.zeros((P, cap), dtype=torch.uint8, device=dev),
                       stats=torch.zeros((P, 4), dtype=i32, device=dev), chi2=torch.zeros((P, 2), dtype=torch.float64, device=dev),
                       median=torch.zeros((P,), dtype=f32, device=dev))
        c8 = None if cam8 is None else np.ascontiguousarray(cam8, np.float32)
        assert c8 is None or c8.size == 8
        st = stream_arg(stream)
        check(self._L.morb_create_initial_map_monocular_batch(
            self._h, C.byref(params), ptr(c8), int(bool(kb8)), P, cap, ptr(img1), ptr(img2), ptr(count), ptr(kps), ptr(matches12), ptr(ok),
            ptr(T21), ptr(P3D), ptr(triangulated), int(nIterations), int(bool(robust)), float(depthScale), int(minTracked), ptr(stop),
            ptr(out["status"]), ptr(out["Tcw2"]), ptr(out["mpPos"]), ptr(out["mpNormal"]), ptr(out["mpDist"]), ptr(out["hasMP"]),
            ptr(out["stats"]), ptr(out["chi2"]), ptr(out["median"]), st))
        return out

    # ---- visual-inertial tracking and mapping ---------------------------------------------------
    def InertialOptimization(self, kfStart, kfState, hasLink, pre, mode, flags=None, prior2=None, global16=None, cap=None, out=None,
                             stream=None):
        """Batched Optimizer::InertialOptimization (morb_inertial_optimization_batch).  Device tensors, P problems: kfStart i32 [P + 1]
        (problem p owns the keyframe rows [kfStart[p], kfStart[p + 1]) in temporal order), kfState f32 [K, 21] (Rwb, twb, velocity, gyro
        bias, acc bias; in / out), hasLink u8 [K], pre f32 [K, 310] (morb_imu_preintegrated records; row k = the link k - 1 -> k), flags
        i32 [P] (bit 0 bMono, bit 1 bFixedVel; mode 0), prior2 f32 [P, 2] (priorG, priorA; modes 0 and 1), global16 f64 [P, 16] (Rwg,
        scale, bg, ba; in / out).  mode: 0 = (Rwg, scale, bg, ba, bMono, ..., priorG, priorA), 1 = (bg, ba, priorG, priorA), 2 = (Rwg,
        scale).  cap = an upper bound of the keyframes of one problem (default: read back from kfStart, which waits for the device).
        Returns (reintegrate u8 [K], stats i32 [P, 4] = outer iterations, LM trials, ok, links; chi2 f64 [P, 2] = before, after); kfState
        and global16 are updated in place."""
        import torch
        P = kfStart.shape[0] - 1
        K = kfState.shape[0]
        if cap is None:
            ks = kfStart.cpu().numpy()
            cap = max(1, int((ks[1:] - ks[:-1]).max()))
        if out is None:
            out = (torch.zeros((K,), dtype=torch.uint8, device=kfState.device),
                   torch.zeros((P, 4), dtype=torch.int32, device=kfState.device),
                   torch.zeros((P, 2), dtype=torch.float64, device=kfState.device))
        st = stream_arg(stream)
        check(self._L.morb_inertial_optimization_batch(self._h, P, int(cap), ptr(kfStart), ptr(kfState), ptr(hasLink), ptr(pre), int(mode),
                                                       ptr(flags), ptr(prior2), ptr(global16), ptr(out[0]), ptr(out[1]), ptr(out[2]), st))
        return out

    def PreintegrateIMU(self, start, acc, gyro, dt, bias, nga, walk, out=None, stream=None):
        """IMU::Preintegrated::Initialize + IntegrateNewMeasurement for many measurement sequences at once.
        Device tensors: start i32 [S+1] (sequence s owns measurements start[s]:start[s+1]), acc / gyro f32 [M, 3],
        dt f32 [M], bias f32 [S, 6] (bax bay baz bwx bwy bwz).  nga / walk: 6 floats each (diagonals of Calib::Cov /
        CovWalk).  Returns f32 [S, PREINT_FLOATS] (morb_imu_preintegrated records, see PREINT_FIELDS)."""
        import torch
        S = start.shape[0] - 1
        if out is None:
            out = torch.empty((S, PREINT_FLOATS), dtype=torch.float32, device=acc.device)
        a = [np.ascontiguousarray(x, np.float32) for x in (nga, walk)]
        st = stream_arg(stream)
        check(self._L.morb_imu_preintegrate_batch(self._h, S, ptr(start), ptr(acc), ptr(gyro), ptr(dt), ptr(bias), ptr(a[0]), ptr(a[1]),
                                                  ptr(out), st))
        return out

    def PoseInertialOptimizationLastKeyFrame(self, hasMP, obs, invSigma2, Xw, close, cam, Tbc, kfState, pre, state, bRecInit=False,
                                             count=None, want_prior=True, out=None, stream=None, rig=None, nLeft=None):
        """Batched Optimizer::PoseInertialOptimizationLastKeyFrame.  Device tensors as PoseOptimization plus close u8
        [F, cap] (mTrackDepth < 10), kfState f32 [F, 21] (fixed), pre f32 [F, PREINT_FLOATS], state f32 [F, 21] in/out
        (Rwb row-major, twb, velocity, gyro bias, acc bias).  Tbc: 12 floats (rotation row-major + translation).
        Returns (nInliers i32 [F], outlier u8 [F, cap], prior f64 [F, 246] or None)."""
        import torch
        F, cap = hasMP.shape
        if out is None:
            out = (torch.empty((F,), dtype=torch.int32, device=hasMP.device),
                   torch.zeros((F, cap), dtype=torch.uint8, device=hasMP.device),
                   torch.empty((F, 246), dtype=torch.float64, device=hasMP.device) if want_prior else None)
        t = np.ascontiguousarray(Tbc, np.float32)
        assert t.size == 12 and pre.shape[1] == PREINT_FLOATS and state.shape[1] == 21 and kfState.shape[1] == 21
        st = stream_arg(stream)
        if rig is not None:   # fisheye rig: rig = 28 floats (see morb_hip.h), nLeft i32 [F] on the device; cam is ignored
            r28 = np.ascontiguousarray(rig, np.float32)
            assert r28.size == 28 and nLeft is not None
            check(self._L.morb_pose_inertial_optimization_last_keyframe_fisheye_batch(
                self._h, F, cap, ptr(count), ptr(nLeft), ptr(hasMP), ptr(obs), ptr(invSigma2), ptr(Xw), ptr(close), ptr(r28), ptr(t),
                ptr(kfState), ptr(pre), int(bool(bRecInit)), ptr(state), ptr(out[1]), ptr(out[0]), ptr(out[2]), st))
            return out
        check(self._L.morb_pose_inertial_optimization_last_keyframe_batch(
            self._h, F, cap, ptr(count), ptr(hasMP), ptr(obs), ptr(invSigma2), ptr(Xw), ptr(close), cam["fx"], cam["fy"], cam["cx"],
            cam["cy"], cam["bf"], ptr(t), ptr(kfState), ptr(pre), int(bool(bRecInit)), ptr(state), ptr(out[1]), ptr(out[0]),
            ptr(out[2]), st))
        return out

    def PoseInertialOptimizationLastFrame(self, hasMP, obs, invSigma2, Xw, close, cam, Tbc, prevState, preFrame, preKF, prevPrior, state,
                                          bRecInit=False, count=None, want_prior=True, out=None, stream=None, rig=None, nLeft=None):
        """Batched Optimizer::PoseInertialOptimizationLastFrame: as PoseInertialOptimizationLastKeyFrame, but the previous
        frame's state (prevState f32 [F, 21]) is free and carries the prior prevPrior f64 [F, 246] (a previous call's third
        result); preFrame = preintegration since the previous frame, preKF = since the last keyframe."""
        import torch
        F, cap = hasMP.shape
        if out is None:
            out = (torch.empty((F,), dtype=torch.int32, device=hasMP.device),
                   torch.zeros((F, cap), dtype=torch.uint8, device=hasMP.device),
                   torch.empty((F, 246), dtype=torch.float64, device=hasMP.device) if want_prior else None)
        t = np.ascontiguousarray(Tbc, np.float32)
        assert t.size == 12 and preFrame.shape[1] == PREINT_FLOATS and preKF.shape[1] == PREINT_FLOATS
        assert state.shape[1] == 21 and prevState.shape[1] == 21 and prevPrior.shape[1] == 246 and prevPrior.dtype == torch.float64
        st = stream_arg(stream)
        if rig is not None:
            r28 = np.ascontiguousarray(rig, np.float32)
            assert r28.size == 28 and nLeft is not None
            check(self._L.morb_pose_inertial_optimization_last_frame_fisheye_batch(
                self._h, F, cap, ptr(count), ptr(nLeft), ptr(hasMP), ptr(obs), ptr(invSigma2), ptr(Xw), ptr(close), ptr(r28), ptr(t),
                ptr(prevState), ptr(preFrame), ptr(preKF), ptr(prevPrior), int(bool(bRecInit)), ptr(state), ptr(out[1]), ptr(out[0]),
                ptr(out[2]), st))
            return out
        check(self._L.morb_pose_inertial_optimization_last_frame_batch(
            self._h, F, cap, ptr(count), ptr(hasMP), ptr(obs), ptr(invSigma2), ptr(Xw), ptr(close), cam["fx"], cam["fy"], cam["cx"],
            cam["cy"], cam["bf"], ptr(t), ptr(prevState), ptr(preFrame), ptr(preKF), ptr(prevPrior), int(bool(bRecInit)), ptr(state),
            ptr(out[1]), ptr(out[0]), ptr(out[2]), st))
        return out

    def LocalInertialBA(self, kfState, kfKind, mpPos, mpClose, eKF, eMP, eObs, eInvSigma2, iKF1, iKF2, iPre, iRobust, iInfoScale, cam, Tbc,
                        bLarge=False, rig=None, eRight=None):
        """Optimizer::LocalInertialBA on host numpy arrays (see morb_local_inertial_ba).  iPre: float32 [nI, PREINT_FLOATS].
        Returns (kfState, mpPos, eraseFlag, stats) with stats = (outer LM iterations, LM trials, ok)."""
        a = [np.ascontiguousarray(kfState, np.float32).copy(), np.ascontiguousarray(kfKind, np.uint8),
             np.ascontiguousarray(mpPos, np.float32).copy(), np.ascontiguousarray(mpClose, np.uint8),
             np.ascontiguousarray(eKF, np.int32), np.ascontiguousarray(eMP, np.int32), np.ascontiguousarray(eObs, np.float32),
             np.ascontiguousarray(eInvSigma2, np.float32), np.ascontiguousarray(iKF1, np.int32), np.ascontiguousarray(iKF2, np.int32),
             np.ascontiguousarray(iPre, np.float32), np.ascontiguousarray(iRobust, np.uint8), np.ascontiguousarray(iInfoScale, np.float32),
             np.ascontiguousarray(Tbc, np.float32)]
        nI = len(a[8])
        assert a[10].shape == (nI, PREINT_FLOATS) and a[0].shape[1] == 21 and a[6].shape[1] == 3
        erase = np.zeros(len(a[4]), np.uint8); stats = np.zeros(3, np.int32)
        if rig is not None:   # fisheye rig: rig = 28 floats, eRight uint8 [nE]; cam is ignored
            r28 = np.ascontiguousarray(rig, np.float32); er = np.ascontiguousarray(eRight, np.uint8)
            assert r28.size == 28 and len(er) == len(a[4])
            check(self._L.morb_local_inertial_ba_fisheye(self._h, len(a[0]), ptr(a[0]), ptr(a[1]), len(a[2]), ptr(a[2]), ptr(a[3]), len(a[4]),
                                                         ptr(a[4]), ptr(a[5]), ptr(a[6]), ptr(er), ptr(a[7]), nI, ptr(a[8]), ptr(a[9]),
                                                         ptr(a[10]), ptr(a[11]), ptr(a[12]), ptr(r28), ptr(a[13]), int(bool(bLarge)),
                                                         ptr(erase), ptr(stats)))
            return a[0], a[2], erase, stats
        check(self._L.morb_local_inertial_ba(self._h, len(a[0]), ptr(a[0]), ptr(a[1]), len(a[2]), ptr(a[2]), ptr(a[3]), len(a[4]), ptr(a[4]),
                                             ptr(a[5]), ptr(a[6]), ptr(a[7]), nI, ptr(a[8]), ptr(a[9]), ptr(a[10]), ptr(a[11]), ptr(a[12]),
                                             cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["bf"], ptr(a[13]), int(bool(bLarge)),
                                             ptr(erase), ptr(stats)))
        return a[0], a[2], erase, stats

    def LocalBundleAdjustment(self, kfPose, kfFixed, mpPos, eKF, eMP, eObs, eInvSigma2, cam, inertial=False, stop=False, mode=0,
                              rig=None):
        """One-shot LocalBundleAdjustment on host numpy arrays; returns (kfPose, mpPos, eraseFlag, stats)."""
        p = BAProblem(self, kfPose, kfFixed, mpPos, eKF, eMP, eObs, eInvSigma2, cam, inertial, rig=rig)
        p.set_mode(mode)
        if stop:
            p.set_stop(True)
        p.solve()
        return p.results()

    def MergeBundleAdjustment(self, kfPose, kfFixed, mpPos, eKF, eMP, eObs, eInvSigma2, cam, stop_flag=None, camL=None):
        """Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag), the welding bundle adjustment of map merging, on
        host numpy arrays (see morb_merge_bundle_adjustment).  camL = 8 floats selects the KannalaBrandt8 left camera (eObs is then
        [nE, 2]; cam is ignored).  stop_flag: a one-byte numpy array standing for `bool* pbStopFlag`.
        Returns (kfPose, mpPos, eraseFlag, levelFlag, stats6)."""
        a = [np.ascontiguousarray(kfPose, np.float32).copy(), np.ascontiguousarray(kfFixed, np.uint8),
             np.ascontiguousarray(mpPos, np.float32).copy(), np.ascontiguousarray(eKF, np.int32), np.ascontiguousarray(eMP, np.int32),
             np.ascontiguousarray(eObs, np.float32), np.ascontiguousarray(eInvSigma2, np.float32)]
        nE = len(a[3])
        erase = np.zeros(nE, np.uint8); level = np.zeros(nE, np.uint8); stats = np.zeros(6, np.int32)
        st = ptr(stop_flag) if stop_flag is not None else None
        if camL is not None:
            c8 = np.ascontiguousarray(camL, np.float32)
            assert c8.size == 8 and a[5].shape == (nE, 2)
            check(self._L.morb_merge_bundle_adjustment_fisheye(self._h, len(a[0]), ptr(a[0]), ptr(a[1]), len(a[2]), ptr(a[2]), nE, ptr(a[3]),
                                                               ptr(a[4]), ptr(a[5]), ptr(a[6]), ptr(c8), st, ptr(erase), ptr(level), ptr(stats)))
            return a[0], a[2], erase, level, stats
        assert a[5].shape == (nE, 3)
        check(self._L.morb_merge_bundle_adjustment(self._h, len(a[0]), ptr(a[0]), ptr(a[1]), len(a[2]), ptr(a[2]), nE, ptr(a[3]), ptr(a[4]),
                                                   ptr(a[5]), ptr(a[6]), cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["bf"], st,
                                                   ptr(erase), ptr(level), ptr(stats)))
        return a[0], a[2], erase, level, stats

    def OptimizeEssentialGraph(self, kfSim3, kfFlags, eI, eJ, eSji, mpPos=None, mpRef=None):
        """Optimizer::OptimizeEssentialGraph, the Sim3 pose graph of loop closing, on host numpy arrays (see morb_optimize_essential_graph).
        kfSim3: float64 [nKF, 8] (qx qy qz qw tx ty tz s); kfFlags: bit 0 fixed, bit 1 _fix_scale; edges (eI, eJ) with measurements eSji
        [nE, 8] in insertion order; mpPos float32 [nMP, 3] with mpRef = the vertex each point is corrected through (-1: left alone), or None.
        Returns (kfSim3, mpPos, stats4, chi2): stats4 = outer iterations, trials, vertices in the system, envelope blocks."""
        S = np.ascontiguousarray(kfSim3, np.float64).reshape(-1, 8).copy()
        fl = np.ascontiguousarray(kfFlags, np.uint8)
        ei, ej = np.ascontiguousarray(eI, np.int32), np.ascontiguousarray(eJ, np.int32)
        M = np.ascontiguousarray(eSji, np.float64).reshape(-1, 8)
        assert len(fl) == len(S) and len(ei) == len(ej) == len(M)
        mp = np.zeros((0, 3), np.float32) if mpPos is None else np.ascontiguousarray(mpPos, np.float32).reshape(-1, 3).copy()
        ref = np.zeros(0, np.int32) if mpRef is None else np.ascontiguousarray(mpRef, np.int32)
        assert len(ref) == len(mp)
        stats, chi2 = np.zeros(4, np.int32), np.zeros(2, np.float64)
        check(self._L.morb_optimize_essential_graph(self._h, len(S), ptr(S), ptr(fl), len(ei), ptr(ei), ptr(ej), ptr(M), len(mp),
                                                    ptr(mp) if len(mp) else None, ptr(ref) if len(mp) else None, ptr(stats), ptr(chi2)))
        return S, mp, stats, chi2

    def OptimizeEssentialGraphMerge(self, kfLists, kfTcw, kfTwc, kfTcwBefMerge, kfTwcBefMerge, cI, cJ, mpPos=None, mpRef=None):
        """The second overload of Optimizer::OptimizeEssentialGraph, the Sim3 pose graph of map merging, on host numpy arrays (see
        morb_optimize_essential_graph_merge).  kfLists: uint8 [nKF], bit 0 vpFixedKFs, bit 1 vpFixedCorrectedKFs, bit 2 vpNonFixedKFs; the
        four poses float32 [nKF, 7] (unit quaternion xyzw, translation); candidate edges (cI, cJ) in insertion order; mpPos float32
        [nMP, 3] with mpRef = the vertex of each point's reference keyframe (-1: left alone), or None.  Returns a dict: kfTcw, kfTwc,
        kfTcwBefMerge, kfTwcBefMerge, mpPos, cKept (1 where the good / bad rule keeps the candidate), stats4, chi2."""
        lists = np.ascontiguousarray(kfLists, np.uint8)
        poses = [np.ascontiguousarray(a, np.float32).reshape(-1, 7).copy() for a in (kfTcw, kfTwc, kfTcwBefMerge, kfTwcBefMerge)]
        ci, cj = np.ascontiguousarray(cI, np.int32), np.ascontiguousarray(cJ, np.int32)
        assert all(len(a) == len(lists) for a in poses) and len(ci) == len(cj)
        mp = np.zeros((0, 3), np.float32) if mpPos is None else np.ascontiguousarray(mpPos, np.float32).reshape(-1, 3).copy()
        ref = np.zeros(0, np.int32) if mpRef is None else np.ascontiguousarray(mpRef, np.int32)
        assert len(ref) == len(mp)
        kept, stats, chi2 = np.zeros(len(ci), np.uint8), np.zeros(4, np.int32), np.zeros(2, np.float64)
        some = len(ci) > 0
        check(self._L.morb_optimize_essential_graph_merge(self._h, len(lists), ptr(lists), *[ptr(a) for a in poses], len(ci), ptr(ci) if some else None,
                                                          ptr(cj) if some else None, ptr(kept) if some else None, len(mp), ptr(mp) if len(mp) else None,
                                                          ptr(ref) if len(mp) else None, ptr(stats), ptr(chi2)))
        return dict(kfTcw=poses[0], kfTwc=poses[1], kfTcwBefMerge=poses[2], kfTwcBefMerge=poses[3], mpPos=mp, cKept=kept, stats4=stats, chi2=chi2)

    def OptimizeEssentialGraph4DoF(self, kfPose, kfBody, kfFixed, Tcb12, eI, eJ, eTij, mpPos=None, mpRef=None, kfScw=None):
        """Optimizer::OptimizeEssentialGraph4DoF, the pose graph of loop closing in an inertial map, on host numpy arrays (see
        morb_optimize_essential_graph_4dof).  kfPose: float64 [nKF, 12] (Rcw row-major, tcw); kfBody: [nKF, 12] (Rwb row-major, twb) at
        entry; kfFixed: uint8 [nKF]; Tcb12: float32 [12]; edges (eI, eJ) with measurements eTij [nE, 12] (dRij row-major, dtij) in insertion
        order; mpPos float32 [nMP, 3] with mpRef = the vertex each point is corrected through (-1: left alone) and kfScw [nKF, 8] = vScw at
        entry, or None.  Returns (kfPose, mpPos, stats4, chi2): stats4 = outer iterations, trials, vertices in the system, envelope blocks."""
        P = np.ascontiguousarray(kfPose, np.float64).reshape(-1, 12).copy()
        B = np.ascontiguousarray(kfBody, np.float64).reshape(-1, 12)
        fx = np.ascontiguousarray(kfFixed, np.uint8)
        tcb = np.ascontiguousarray(Tcb12, np.float32).reshape(12)
        ei, ej = np.ascontiguousarray(eI, np.int32), np.ascontiguousarray(eJ, np.int32)
        M = np.ascontiguousarray(eTij, np.float64).reshape(-1, 12)
        assert len(fx) == len(P) == len(B) and len(ei) == len(ej) == len(M)
        mp = np.zeros((0, 3), np.float32) if mpPos is None else np.ascontiguousarray(mpPos, np.float32).reshape(-1, 3).copy()
        ref = np.zeros(0, np.int32) if mpRef is None else np.ascontiguousarray(mpRef, np.int32)
        assert len(ref) == len(mp)
        scw = None
        if len(mp):
            scw = np.ascontiguousarray(kfScw, np.float64).reshape(-1, 8)
            assert len(scw) == len(P)
        stats, chi2 = np.zeros(4, np.int32), np.zeros(2, np.float64)
        check(self._L.morb_optimize_essential_graph_4dof(self._h, len(P), ptr(P), ptr(B), ptr(fx), ptr(tcb), len(ei), ptr(ei), ptr(ej), ptr(M), len(mp),
                                                         ptr(mp) if len(mp) else None, ptr(ref) if len(mp) else None, ptr(scw) if len(mp) else None,
                                                         ptr(stats), ptr(chi2)))
        return P, mp, stats, chi2

    def BundleAdjustment(self, kfPose, kfFixed, mpPos, eKF, eMP, eObs, eInvSigma2, cam, n_iterations=10, robust=False, stop_flag=None,
                         rig=None):
        """Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust), the whole-map bundle adjustment of loop
        closing, on host numpy arrays (see morb_bundle_adjustment).  Pass the keyframes by ascending mnId.  rig = dict(eRight uint8 [nE],
        camL, camR (8 floats each), Trl (7 floats)) selects the KannalaBrandt8 stereo rig (eObs is then [nE, 2]; cam is ignored).
        stop_flag: a one-byte numpy array standing for `bool* pbStopFlag`.
        Returns (kfPose, mpPos, stats4, chi2): stats4 = outer iterations, trials, keyframes in the system, envelope blocks."""
        a = [np.ascontiguousarray(kfPose, np.float32).copy(), np.ascontiguousarray(kfFixed, np.uint8),
             np.ascontiguousarray(mpPos, np.float32).copy(), np.ascontiguousarray(eKF, np.int32), np.ascontiguousarray(eMP, np.int32),
             np.ascontiguousarray(eObs, np.float32), np.ascontiguousarray(eInvSigma2, np.float32)]
        nE = len(a[3])
        assert len(a[1]) == len(a[0]) and len(a[4]) == len(a[6]) == nE
        stats, chi2 = np.zeros(4, np.int32), np.zeros(2, np.float64)
        st = ptr(stop_flag) if stop_flag is not None else None
        if rig is not None:
            er = np.ascontiguousarray(rig["eRight"], np.uint8)
            cl, cr, trl = (np.ascontiguousarray(rig[k], np.float32) for k in ("camL", "camR", "Trl"))
            assert cl.size == 8 and cr.size == 8 and trl.size == 7 and len(er) == nE and a[5].shape == (nE, 2)
            check(self._L.morb_bundle_adjustment_fisheye(self._h, len(a[0]), ptr(a[0]), ptr(a[1]), len(a[2]), ptr(a[2]), nE, ptr(a[3]), ptr(a[4]),
                                                         ptr(a[5]), ptr(er), ptr(a[6]), ptr(cl), ptr(cr), ptr(trl), int(n_iterations),
                                                         int(bool(robust)), st, ptr(stats), ptr(chi2)))
            return a[0], a[2], stats, chi2
        assert a[5].shape == (nE, 3)
        check(self._L.morb_bundle_adjustment(self._h, len(a[0]), ptr(a[0]), ptr(a[1]), len(a[2]), ptr(a[2]), nE, ptr(a[3]), ptr(a[4]), ptr(a[5]),
                                             ptr(a[6]), cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["bf"], int(n_iterations),
                                             int(bool(robust)), st, ptr(stats), ptr(chi2)))
        return a[0], a[2], stats, chi2

    def Sim3LogLibm(self, d, s):
        """acos(d) and log(s) as the device computes them inside Sim3::log (see morb_sim3_log_libm)."""
        d, s = np.ascontiguousarray(d, np.float64), np.ascontiguousarray(s, np.float64)
        assert d.shape == s.shape and d.ndim == 1
        a, l = np.zeros_like(d), np.zeros_like(d)
        check(self._L.morb_sim3_log_libm(self._h, len(d), ptr(d), ptr(s), ptr(a), ptr(l)))
        return a, l

    def MergeInertialBA(self, kfState, kfKind, mpPos, eKF, eMP, eObs, eInvSigma2, iKF1, iKF2, iPre, cam, Tbc, stop_flag=None, rig=None):
        """Optimizer::MergeInertialBA(pCurrKF, pMergeKF, pbStopFlag, pMap, corrPoses), the welding bundle adjustment of an inertial map
        merge, on host numpy arrays (see morb_merge_inertial_ba).  kfKind: 0 free (15 unknowns), 1 fixed with an IMU state, 2 fixed observer,
        3 free in the pose only.  iPre: float32 [nI, PREINT_FLOATS].  rig = 28 floats puts every edge on the left KannalaBrandt8 camera
        (cam is ignored).  stop_flag: a one-byte numpy array standing for `bool* pbStopFlag`.
        Returns (kfState, mpPos, eraseFlag, stats3) with stats3 = (outer LM iterations, LM trials, ran)."""
        a = [np.ascontiguousarray(kfState, np.float32).copy(), np.ascontiguousarray(kfKind, np.uint8),
             np.ascontiguousarray(mpPos, np.float32).copy(), np.ascontiguousarray(eKF, np.int32), np.ascontiguousarray(eMP, np.int32),
             np.ascontiguousarray(eObs, np.float32), np.ascontiguousarray(eInvSigma2, np.float32), np.ascontiguousarray(iKF1, np.int32),
             np.ascontiguousarray(iKF2, np.int32), np.ascontiguousarray(iPre, np.float32).reshape(-1, PREINT_FLOATS),
             np.ascontiguousarray(Tbc, np.float32)]
        nE, nI = len(a[3]), len(a[7])
        assert a[9].shape == (nI, PREINT_FLOATS) and a[0].shape[1] == 21 and a[5].shape == (nE, 3)
        erase = np.zeros(nE, np.uint8); stats = np.zeros(3, np.int32)
        st = ptr(stop_flag) if stop_flag is not None else None
        if rig is not None:
            r28 = np.ascontiguousarray(rig, np.float32)
            assert r28.size == 28
            check(self._L.morb_merge_inertial_ba_fisheye(self._h, len(a[0]), ptr(a[0]), ptr(a[1]), len(a[2]), ptr(a[2]), nE, ptr(a[3]), ptr(a[4]),
                                                         ptr(a[5]), ptr(a[6]), nI, ptr(a[7]), ptr(a[8]), ptr(a[9]), ptr(r28), ptr(a[10]), st,
                                                         ptr(erase), ptr(stats)))
            return a[0], a[2], erase, stats
        check(self._L.morb_merge_inertial_ba(self._h, len(a[0]), ptr(a[0]), ptr(a[1]), len(a[2]), ptr(a[2]), nE, ptr(a[3]), ptr(a[4]), ptr(a[5]),
                                             ptr(a[6]), nI, ptr(a[7]), ptr(a[8]), ptr(a[9]), cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                                             cam["bf"], ptr(a[10]), st, ptr(erase), ptr(stats)))
        return a[0], a[2], erase, stats

    def FullInertialBA(self, kfState, kfKind, mpPos, eKF, eMP, eObs, eInvSigma2, iKF1, iKF2, iPre, cam, Tbc, its=7, init=False, prior_g=1e2,
                       prior_a=1e6, bias6=None, stop_flag=None, rig=None, eRight=None):
        """Optimizer::FullInertialBA(pMap, its, bFixLocal, nLoopId, pbStopFlag, bInit, priorG, priorA), the inertial whole-map bundle
        adjustment, on host numpy arrays (see morb_full_inertial_ba).  Pass the keyframes by ascending mnId.  kfKind: 0 free (15 unknowns; 9
        with init), 1 fixed with an IMU state, 2 fixed observer, 3 free in the pose only.  iPre: float32 [nI, PREINT_FLOATS].  init: one
        shared gyro and accelerometer bias, bias6 (gyro, then accelerometer), with the priors prior_g / prior_a.  rig = 28 floats and eRight
        (uint8 [nE]) select the KannalaBrandt8 rig (cam is ignored).  stop_flag: a one-byte numpy array standing for `bool* pbStopFlag`.
        Returns (kfState, mpPos, bias6, stats4, chi2): stats4 = outer iterations, trials, scalar unknowns, envelope blocks."""
        a = [np.ascontiguousarray(kfState, np.float32).copy(), np.ascontiguousarray(kfKind, np.uint8),
             np.ascontiguousarray(mpPos, np.float32).copy(), np.ascontiguousarray(eKF, np.int32), np.ascontiguousarray(eMP, np.int32),
             np.ascontiguousarray(eObs, np.float32), np.ascontiguousarray(eInvSigma2, np.float32), np.ascontiguousarray(iKF1, np.int32),
             np.ascontiguousarray(iKF2, np.int32), np.ascontiguousarray(iPre, np.float32).reshape(-1, PREINT_FLOATS),
             np.ascontiguousarray(Tbc, np.float32)]
        nE, nI = len(a[3]), len(a[7])
        assert a[9].shape == (nI, PREINT_FLOATS) and a[0].shape[1] == 21 and a[5].shape == (nE, 3)
        b6 = np.ascontiguousarray(bias6, np.float32).copy() if bias6 is not None else np.zeros(6, np.float32)
        assert b6.size == 6 and (bias6 is not None or not init)
        stats, chi2 = np.zeros(4, np.int32), np.zeros(2, np.float64)
        st = ptr(stop_flag) if stop_flag is not None else None
        links = (nI, ptr(a[7]) if nI else None, ptr(a[8]) if nI else None, ptr(a[9]) if nI else None)
        tail = (ptr(a[10]), int(its), int(bool(init)), float(prior_g), float(prior_a), ptr(b6), st, ptr(stats), ptr(chi2))
        if rig is not None:
            r28, er = np.ascontiguousarray(rig, np.float32), np.ascontiguousarray(eRight, np.uint8)
            assert r28.size == 28 and len(er) == nE
            check(self._L.morb_full_inertial_ba_fisheye(self._h, len(a[0]), ptr(a[0]), ptr(a[1]), len(a[2]), ptr(a[2]), nE, ptr(a[3]), ptr(a[4]),
                                                        ptr(a[5]), ptr(er), ptr(a[6]), *links, ptr(r28), *tail))
            return a[0], a[2], b6, stats, chi2
        check(self._L.morb_full_inertial_ba(self._h, len(a[0]), ptr(a[0]), ptr(a[1]), len(a[2]), ptr(a[2]), nE, ptr(a[3]), ptr(a[4]), ptr(a[5]),
                                            ptr(a[6]), *links, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["bf"], *tail))
        return a[0], a[2], b6, stats, chi2


def local_bundle_adjustment_oneshot(opt, kfPose, kfFixed, mpPos, eKF, eMP, eObs, eInvSigma2, cam, inertial=False, stop_flag=None):
    """The one-shot ABI entry (`morb_local_bundle_adjustment`), as the reference binding calls it: `stop_flag` is a one-byte
    numpy array standing for `bool* pbStopFlag` (another thread may set it while the call runs)."""
    L = lib()
    a = [np.ascontiguousarray(kfPose, np.float32).copy(), np.ascontiguousarray(kfFixed, np.uint8),
         np.ascontiguousarray(mpPos, np.float32).copy(), np.ascontiguousarray(eKF, np.int32), np.ascontiguousarray(eMP, np.int32),
         np.ascontiguousarray(eObs, np.float32), np.ascontiguousarray(eInvSigma2, np.float32)]
    erase = np.zeros(len(a[3]), np.uint8); stats = np.zeros(2, np.int32)
    check(L.morb_local_bundle_adjustment(opt._h, len(a[0]), ptr(a[0]), ptr(a[1]), len(a[2]), ptr(a[2]), len(a[3]), ptr(a[3]), ptr(a[4]),
                                         ptr(a[5]), ptr(a[6]), cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["bf"],
                                         1 if inertial else 0, ptr(stop_flag) if stop_flag is not None else None, ptr(erase), ptr(stats)))
    return a[0], a[2], erase, stats


def local_bundle_adjustment_fisheye_oneshot(opt, kfPose, kfFixed, mpPos, eKF, eMP, eObs2, eRight, eInvSigma2, camL, camR, Trl, inertial=False,
                                            stop_flag=None):
    """The one-shot ABI entry on the KannalaBrandt8 rig (`morb_local_bundle_adjustment_fisheye`)."""
    L = lib()
    a = [np.ascontiguousarray(kfPose, np.float32).copy(), np.ascontiguousarray(kfFixed, np.uint8),
         np.ascontiguousarray(mpPos, np.float32).copy(), np.ascontiguousarray(eKF, np.int32), np.ascontiguousarray(eMP, np.int32),
         np.ascontiguousarray(eObs2, np.float32), np.ascontiguousarray(eRight, np.uint8), np.ascontiguousarray(eInvSigma2, np.float32),
         np.ascontiguousarray(camL, np.float32), np.ascontiguousarray(camR, np.float32), np.ascontiguousarray(Trl, np.float32)]
    erase = np.zeros(len(a[3]), np.uint8); stats = np.zeros(2, np.int32)
    check(L.morb_local_bundle_adjustment_fisheye(opt._h, len(a[0]), ptr(a[0]), ptr(a[1]), len(a[2]), ptr(a[2]), len(a[3]), ptr(a[3]), ptr(a[4]),
                                                 ptr(a[5]), ptr(a[6]), ptr(a[7]), ptr(a[8]), ptr(a[9]), ptr(a[10]), 1 if inertial else 0,
                                                 ptr(stop_flag) if stop_flag is not None else None, ptr(erase), ptr(stats)))
    return a[0], a[2], erase, stats


class BAProblem:
    """A LocalBundleAdjustment graph resident in HBM (create once, solve repeatedly).
    rig = dict(eRight uint8 [nE], camL, camR (8 floats each), Trl (7 floats)) selects the KannalaBrandt8 stereo rig
    (eObs is then [nE, 2]; cam is ignored)."""

    def __init__(self, opt, kfPose, kfFixed, mpPos, eKF, eMP, eObs, eInvSigma2, cam, inertial=False, rig=None):
        self._L = lib()
        self._opt = opt
        self._h = C.c_void_p()
        a = [np.ascontiguousarray(kfPose, np.float32), np.ascontiguousarray(kfFixed, np.uint8),
             np.ascontiguousarray(mpPos, np.float32), np.ascontiguousarray(eKF, np.int32), np.ascontiguousarray(eMP, np.int32),
             np.ascontiguousarray(eObs, np.float32), np.ascontiguousarray(eInvSigma2, np.float32)]
        self.nKF, self.nMP, self.nE = len(a[0]), len(a[2]), len(a[3])
        self._init = (a[0], a[2])
        if rig is not None:
            r = [np.ascontiguousarray(rig["eRight"], np.uint8), np.ascontiguousarray(rig["camL"], np.float32),
                 np.ascontiguousarray(rig["camR"], np.float32), np.ascontiguousarray(rig["Trl"], np.float32)]
            assert a[5].shape == (self.nE, 2)
            check(self._L.morb_ba_problem_create_fisheye(opt._h, C.byref(self._h), self.nKF, ptr(a[0]), ptr(a[1]), self.nMP, ptr(a[2]),
                                                         self.nE, ptr(a[3]), ptr(a[4]), ptr(a[5]), ptr(r[0]), ptr(a[6]), ptr(r[1]),
                                                         ptr(r[2]), ptr(r[3]), 1 if inertial else 0))
            return
        check(self._L.morb_ba_problem_create(opt._h, C.byref(self._h), self.nKF, ptr(a[0]), ptr(a[1]), self.nMP, ptr(a[2]),
                                             self.nE, ptr(a[3]), ptr(a[4]), ptr(a[5]), ptr(a[6]), cam["fx"], cam["fy"],
                                             cam["cx"], cam["cy"], cam["bf"], 1 if inertial else 0))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.morb_ba_problem_destroy(self._h)
            self._h = None

    __del__ = close

    def set_mode(self, mode):
        """0 = grid (phase kernels over the whole GPU, default), 1 = one persistent workgroup."""
        check(self._L.morb_ba_set_mode(self._h, int(mode)))

    def schur_profile(self, iters=50):
        """(ms per launch, MFMA flops issued per launch, flops of the sparse block-pair form) of the Schur product."""
        ms = C.c_float(); fl = C.c_double(); uf = C.c_double()
        check(self._L.morb_ba_schur_profile(self._h, int(iters), C.byref(ms), C.byref(fl), C.byref(uf)))
        return ms.value, fl.value, uf.value

    def set_stop(self, on):
        check(self._L.morb_ba_set_stop(self._h, 1 if on else 0))

    def solve(self, stream=None):
        check(self._L.morb_ba_solve(self._h, stream_arg(stream)))

    def results(self):
        kf = self._init[0].copy(); mp = self._init[1].copy()
        erase = np.zeros(self.nE, np.uint8); stats = np.zeros(2, np.int32)
        check(self._L.morb_ba_results(self._h, ptr(kf), ptr(mp), ptr(erase), ptr(stats)))
        return kf, mp, erase, stats
