// The reference's own Optimizer signatures for the hot path (include/Optimizer.h:67-101) as static member templates of
// ORB_SLAM3::Optimizer — included at the end of Optimizer.h.  Templated on Frame / KeyFrame / Map (and through them MapPoint, Sophus,
// IMU::Preintegrated, ConstraintPoseImu) so this header names none of the reference's or its third parties' types: the call sites
//     Optimizer::PoseOptimization(&mCurrentFrame);                                                    Tracking.cc:2559, :2710, :3020, :3026
//     Optimizer::PoseInertialOptimizationLastFrame(&mCurrentFrame) / ...LastKeyFrame(&mCurrentFrame)  Tracking.cc:3032-3041
//     Optimizer::LocalBundleAdjustment(mpCurrentKeyFrame, &mbAbortBA, mpCurrentKeyFrame->GetMap(), a, b, c, d);              LocalMapping.cc:181
//     Optimizer::LocalInertialBA(mpCurrentKeyFrame, &mbAbortBA, mpCurrentKeyFrame->GetMap(), a, b, c, d, bLarge, !...GetIniertialBA2());  :173
//     Optimizer::LocalBundleAdjustment(mpCurrentKF, vpLocalCurrentWindowKFs, vpMergeConnectedKFs, &bStop);                 LoopClosing.cc:1652
// compile unchanged.  Each member assembles the graph exactly as the reference's method does (same selection loops, same flags written to
// mnBALocalForKF / mnBAFixedForKF, same locks), hands it flattened to the C ABI, and writes the result back as the reference does.
// KannalaBrandt8 rigs (mpCamera2 != NULL) dispatch to the *_fisheye entry points.  See reference_glue.h for what has been compiled.
#pragma once
#include <cmath>
#include <cstring>
#include <list>
#include <map>
#include <set>
#include <tuple>

#include "reference_glue.h"

namespace ORB_SLAM3 {
namespace morb_glue {

// IMU::Preintegrated (include/ImuTypes.h:154-263) -> the plain record of morb_hip.h
template <class Pre>
inline void fill_pre(morb_imu_preintegrated& o, const Pre* p) {
  auto m3 = [](float* d, const auto& M) { for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) d[3 * r + c] = M(r, c); };
  auto v3 = [](float* d, const auto& V) { for (int k = 0; k < 3; ++k) d[k] = V(k); };
  o.dT = p->dT;
  m3(o.dR, p->dR); v3(o.dV, p->dV); v3(o.dP, p->dP);
  m3(o.JRg, p->JRg); m3(o.JVg, p->JVg); m3(o.JVa, p->JVa); m3(o.JPg, p->JPg); m3(o.JPa, p->JPa);
  for (int r = 0; r < 15; ++r) for (int c = 0; c < 15; ++c) o.C[15 * r + c] = p->C(r, c);
  o.b[0] = p->b.bax; o.b[1] = p->b.bay; o.b[2] = p->b.baz; o.b[3] = p->b.bwx; o.b[4] = p->b.bwy; o.b[5] = p->b.bwz;
  for (int k = 0; k < 6; ++k) { o.nga[k] = p->Nga.diagonal()(k); o.ngaWalk[k] = p->NgaWalk.diagonal()(k); }
  v3(o.avgA, p->avgA); v3(o.avgW, p->avgW);
}
// Rwb (row-major), twb, velocity, gyro bias, acc bias of a Frame / KeyFrame (VertexPose / VertexVelocity / VertexGyroBias / VertexAccBias
// constructors, G2oTypes.h:128-199)
template <class F>
inline void imu_state21(F* f, float s[21]) {
  const auto R = f->GetImuRotation();
  const auto t = f->GetImuPosition();
  const auto v = f->GetVelocity();
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) s[3 * r + c] = R(r, c);
  for (int k = 0; k < 3; ++k) { s[9 + k] = t(k); s[12 + k] = v(k); }
}
template <class B> inline void bias6(const B& b, float* s15) { s15[0] = b.bwx; s15[1] = b.bwy; s15[2] = b.bwz; s15[3] = b.bax; s15[4] = b.bay; s15[5] = b.baz; }
template <class SE3> inline void tbc12(const SE3& Tbc, float o[12]) {
  const auto R = Tbc.rotationMatrix(); const auto t = Tbc.translation();
  for (int r = 0; r < 3; ++r) { o[9 + r] = t(r); for (int c = 0; c < 3; ++c) o[3 * r + c] = R(r, c); }
}
// rig28 = left KB8 parameters (8), right ones (8), rotation (9, row-major) and translation (3) of GetRelativePoseTrl()
template <class F> inline void rig28(F* f, float o[28]) {
  cam8(f->mpCamera, o); cam8(f->mpCamera2, o + 8);
  tbc12(f->GetRelativePoseTrl(), o + 16);
}
// ConstraintPoseImu (include/G2oTypes.h:706-729) <-> the 246 doubles of morb_hip.h: Rwb (9, row-major), twb, vwb, bg, ba, H (15 x 15, row-major)
template <class CPI> inline void prior_to_doubles(const CPI* c, double* o) {
  for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) o[3 * r + k] = c->Rwb(r, k);
  for (int k = 0; k < 3; ++k) { o[9 + k] = c->twb(k); o[12 + k] = c->vwb(k); o[15 + k] = c->bg(k); o[18 + k] = c->ba(k); }
  for (int r = 0; r < 15; ++r) for (int k = 0; k < 15; ++k) o[21 + 15 * r + k] = c->H(r, k);
}
template <class CPI> inline CPI* prior_from_doubles(const double* o) {
  typename std::decay<decltype(CPI::Rwb)>::type R;
  typename std::decay<decltype(CPI::twb)>::type t, v, bg, ba;
  typename std::decay<decltype(CPI::H)>::type H;
  for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) R(r, k) = o[3 * r + k];
  for (int k = 0; k < 3; ++k) { t(k) = o[9 + k]; v(k) = o[12 + k]; bg(k) = o[15 + k]; ba(k) = o[18 + k]; }
  for (int r = 0; r < 15; ++r) for (int k = 0; k < 15; ++k) H(r, k) = o[21 + 15 * r + k];
  return new CPI(R, t, v, bg, ba, H);   // (the constructor's eigenvalue clamp runs again on the already clamped matrix)
}

// the visual edges of one frame as the pose optimisers build them (Optimizer.cc:806-946, :4444-4528): feature i with a map point ->
// (x, y, uRight or -1), 1 / sigma^2 of its octave, the point's world position; on a rig features [0, Nleft) are left-camera observations
// (mvKeys), the rest right-camera ones (mvKeysRight), all monocular
template <class FrameT>
struct FrameEdges {
  int N = 0, nLeft = -1;
  std::vector<uint8_t> has, close, outlier;
  std::vector<float> obs, inv, Xw;
  explicit FrameEdges(FrameT* pFrame) {
    using MP = typename std::remove_pointer<typename std::decay<decltype(pFrame->mvpMapPoints[0])>::type>::type;
    N = pFrame->N; nLeft = pFrame->Nleft;
    has.assign(N, 0); close.assign(N, 0); obs.assign((size_t)N * 3, 0.f); inv.assign(N, 0.f); Xw.assign((size_t)N * 3, 0.f);
    outlier.assign(pFrame->mvbOutlier.begin(), pFrame->mvbOutlier.end());
    outlier.resize(N, 0);
    std::unique_lock<std::mutex> lock(MP::mGlobalMutex);   // :806, :4445
    for (int i = 0; i < N; ++i) {
      MP* pMP = pFrame->mvpMapPoints[i];
      if (!pMP) continue;
      has[i] = 1; outlier[i] = 0;                          // :817, :860: pFrame->mvbOutlier[i] = false
      const auto& kp = nLeft == -1 ? pFrame->mvKeysUn[i] : (i < nLeft ? pFrame->mvKeys[i] : pFrame->mvKeysRight[i - nLeft]);
      obs[3 * i] = kp.pt.x; obs[3 * i + 1] = kp.pt.y; obs[3 * i + 2] = nLeft == -1 ? pFrame->mvuRight[i] : -1.f;   // < 0: monocular edge (:811)
      inv[i] = pFrame->mvInvLevelSigma2[kp.octave];
      close[i] = pMP->mTrackDepth < 10.f ? 1 : 0;          // :4576 bClose
      const auto X = pMP->GetWorldPos();
      for (int k = 0; k < 3; ++k) Xw[3 * i + k] = X(k);
    }
  }
  void write_outliers(FrameT* pFrame) const { for (int i = 0; i < N; ++i) pFrame->mvbOutlier[i] = outlier[i] != 0; }
};

}  // namespace morb_glue

// int Optimizer::PoseOptimization(Frame* pFrame)  Optimizer.cc:762-1051
template <class FrameT>
int Optimizer::PoseOptimization(FrameT* pFrame) {
  using SE3 = typename std::decay<decltype(pFrame->GetPose())>::type;
  morb_glue::FrameEdges<FrameT> fe(pFrame);
  PoseOptimizationView f;
  f.N = fe.N; f.hasMapPoint = fe.has.data(); f.obs = fe.obs.data(); f.invSigma2 = fe.inv.data(); f.worldPos = fe.Xw.data();
  f.mvbOutlier = fe.outlier;
  f.fx = pFrame->fx; f.fy = pFrame->fy; f.cx = pFrame->cx; f.cy = pFrame->cy; f.mbf = pFrame->mbf;
  morb_glue::pose7(pFrame->GetPose(), f.pose);                     // :781-783
  float rigp[28];
  if (pFrame->mpCamera2) { morb_glue::rig28(pFrame, rigp); f.nLeft = pFrame->Nleft; f.rig28 = rigp; }   // :880-946
  int nInitialCorrespondences = 0;
  for (int i = 0; i < fe.N; ++i) nInitialCorrespondences += fe.has[i] ? 1 : 0;
  if (fe.N <= 0 || nInitialCorrespondences < 3) {                   // :951: the reference returns without touching the pose; the graph fill
    fe.write_outliers(pFrame);                                      // before it has already cleared mvbOutlier[i] of the features with a map point
    return 0;
  }
  const int nin = PoseOptimization(f);
  pFrame->SetPose(morb_glue::make_se3<SE3>(f.pose));               // :1044-1048
  fe.outlier = f.mvbOutlier;
  fe.write_outliers(pFrame);
  return nin;
}

// int Optimizer::PoseInertialOptimizationLastKeyFrame(Frame* pFrame, bool bRecInit)  Optimizer.cc:4391-4757
template <class FrameT>
int Optimizer::PoseInertialOptimizationLastKeyFrame(FrameT* pFrame, bool bRecInit) {
  using CPI = typename std::remove_pointer<decltype(pFrame->mpcpi)>::type;
  using Bias = typename std::decay<decltype(pFrame->mImuBias)>::type;
  morb_glue::FrameEdges<FrameT> fe(pFrame);
  PoseInertialView v;
  v.N = fe.N; v.nLeft = fe.nLeft; v.hasMapPoint = fe.has.data(); v.obs = fe.obs.data(); v.invSigma2 = fe.inv.data(); v.worldPos = fe.Xw.data();
  v.close = fe.close.data(); v.mvbOutlier = fe.outlier;
  v.fx = pFrame->fx; v.fy = pFrame->fy; v.cx = pFrame->cx; v.cy = pFrame->cy; v.mbf = pFrame->mbf;
  float rigp[28];
  if (pFrame->mpCamera2) { morb_glue::rig28(pFrame, rigp); v.rig28 = rigp; }
  morb_glue::tbc12(pFrame->mImuCalib.mTbc, v.Tbc12);
  morb_glue::imu_state21(pFrame, v.state); morb_glue::bias6(pFrame->mImuBias, v.state + 15);          // VertexPose(pFrame), ... :4411-4426
  auto* pKF = pFrame->mpLastKeyFrame;                                                                  // :4548-4566: fixed vertices
  morb_glue::imu_state21(pKF, v.otherState); morb_glue::bias6(pKF->GetImuBias(), v.otherState + 15);
  morb_glue::fill_pre(v.pre, pFrame->mpImuPreintegrated);
  const int nin = PoseInertialOptimizationLastKeyFrame(v, bRecInit);
  write_back_inertial(pFrame, v);
  pFrame->mImuBias = Bias(v.state[18], v.state[19], v.state[20], v.state[15], v.state[16], v.state[17]);   // :4708-4710
  pFrame->mpcpi = morb_glue::prior_from_doubles<CPI>(v.prior);                                        // :4752-4754
  fe.outlier = v.mvbOutlier; fe.write_outliers(pFrame);
  return nin;
}

// int Optimizer::PoseInertialOptimizationLastFrame(Frame* pFrame, bool bRecInit)  Optimizer.cc:4761-5161
template <class FrameT>
int Optimizer::PoseInertialOptimizationLastFrame(FrameT* pFrame, bool bRecInit) {
  using CPI = typename std::remove_pointer<decltype(pFrame->mpcpi)>::type;
  using Bias = typename std::decay<decltype(pFrame->mImuBias)>::type;
  FrameT* pFp = pFrame->mpPrevFrame;                                                                   // :4920
  if (pFp->mpcpi == nullptr) return 0;                                                                 // :4968-4971 "NO MPCPI"
  morb_glue::FrameEdges<FrameT> fe(pFrame);
  PoseInertialView v;
  v.N = fe.N; v.nLeft = fe.nLeft; v.hasMapPoint = fe.has.data(); v.obs = fe.obs.data(); v.invSigma2 = fe.inv.data(); v.worldPos = fe.Xw.data();
  v.close = fe.close.data(); v.mvbOutlier = fe.outlier;
  v.fx = pFrame->fx; v.fy = pFrame->fy; v.cx = pFrame->cx; v.cy = pFrame->cy; v.mbf = pFrame->mbf;
  float rigp[28];
  if (pFrame->mpCamera2) { morb_glue::rig28(pFrame, rigp); v.rig28 = rigp; }
  morb_glue::tbc12(pFrame->mImuCalib.mTbc, v.Tbc12);
  morb_glue::imu_state21(pFrame, v.state); morb_glue::bias6(pFrame->mImuBias, v.state + 15);
  morb_glue::imu_state21(pFp, v.otherState); morb_glue::bias6(pFp->mImuBias, v.otherState + 15);      // :4922-4937: free vertices of the previous frame
  morb_glue::fill_pre(v.pre, pFrame->mpImuPreintegratedFrame);                                        // :4939 EdgeInertial
  morb_glue::fill_pre(v.preKF, pFrame->mpImuPreintegrated);                                           // :4951-4965 random-walk information
  morb_glue::prior_to_doubles(pFp->mpcpi, v.prevPrior);                                               // :4972 EdgePriorPoseImu
  const int nin = PoseInertialOptimizationLastFrame(v, bRecInit);
  write_back_inertial(pFrame, v);
  pFrame->mImuBias = Bias(v.state[18], v.state[19], v.state[20], v.state[15], v.state[16], v.state[17]);   // :5078-5080
  pFrame->mpcpi = morb_glue::prior_from_doubles<CPI>(v.prior);                                        // :5150-5152
  static CPI* oldMpcpi = nullptr;                                                                     // :4759, :5153-5159: the fork's guard against freeing the same
  if (oldMpcpi != pFp->mpcpi) {                                                                       // address twice ("SAME MPCPI": nothing is deleted, the pointer stays)
    oldMpcpi = pFp->mpcpi;
    delete pFp->mpcpi;
    pFp->mpcpi = NULL;
  }
  fe.outlier = v.mvbOutlier; fe.write_outliers(pFrame);
  return nin;
}
template <class FrameT>
void Optimizer::write_back_inertial(FrameT* pFrame, const PoseInertialView& v) {
  // pFrame->SetImuPoseVelocity(VP->estimate().Rwb.cast<float>(), VP->estimate().twb.cast<float>(), VV->estimate().cast<float>())  :4703-4705
  typename std::decay<decltype(pFrame->GetImuRotation())>::type R;
  typename std::decay<decltype(pFrame->GetImuPosition())>::type t, vel;
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R(r, c) = v.state[3 * r + c];
  for (int k = 0; k < 3; ++k) { t(k) = v.state[9 + k]; vel(k) = v.state[12 + k]; }
  pFrame->SetImuPoseVelocity(R, t, vel);
}

// void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs, int& num_edges)
// Optimizer.cc:1053-1441
template <class KF, class MapT>
void Optimizer::LocalBundleAdjustment(KF* pKF, bool* pbStopFlag, MapT* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs, int& num_edges) {
  using SE3 = typename std::decay<decltype(pKF->GetPose())>::type;
  using MP = typename std::remove_pointer<typename std::decay<decltype(pKF->GetMapPointMatches()[0])>::type>::type;
  // :1058-1122 — the reference's graph selection, unchanged
  std::list<KF*> lLocalKeyFrames;
  lLocalKeyFrames.push_back(pKF);
  pKF->mnBALocalForKF = pKF->mnId;
  MapT* pCurrentMap = pKF->GetMap();
  const std::vector<KF*> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
  for (KF* pKFi : vNeighKFs) {
    pKFi->mnBALocalForKF = pKF->mnId;
    if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) lLocalKeyFrames.push_back(pKFi);
  }
  num_fixedKF = 0;
  std::list<MP*> lLocalMapPoints;
  for (KF* pKFi : lLocalKeyFrames) {
    if (pKFi->mnId == pMap->GetInitKFid()) num_fixedKF = 1;
    for (MP* pMP : pKFi->GetMapPointMatches())
      if (pMP && !pMP->isBad() && pMP->GetMap() == pCurrentMap && pMP->mnBALocalForKF != pKF->mnId) {
        lLocalMapPoints.push_back(pMP);
        pMP->mnBALocalForKF = pKF->mnId;
      }
  }
  std::list<KF*> lFixedCameras;
  for (MP* pMP : lLocalMapPoints)
    for (const auto& ob : pMP->GetObservations()) {
      KF* pKFi = ob.first;
      if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
        pKFi->mnBAFixedForKF = pKF->mnId;
        if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) lFixedCameras.push_back(pKFi);
      }
    }
  num_fixedKF = (int)lFixedCameras.size() + num_fixedKF;
  if (num_fixedKF == 0) return;   // :1118-1122 "LBA aborted"
  // :1150-1351 — vertices and edges, flattened
  const bool rig = pKF->mpCamera2 != nullptr;
  std::map<KF*, int> kfIndex;
  std::vector<KF*> kfs;
  std::vector<float> kfPose;
  std::vector<uint8_t> kfFixed;
  auto add_kf = [&](KF* k, bool fixed) {
    kfIndex[k] = (int)kfs.size(); kfs.push_back(k);
    float p[7];
    morb_glue::pose7(k->GetPose(), p);
    kfPose.insert(kfPose.end(), p, p + 7);
    kfFixed.push_back(fixed ? 1 : 0);
  };
  for (KF* k : lLocalKeyFrames) add_kf(k, k->mnId == pMap->GetInitKFid());   // :1160
  num_OptKF = (int)lLocalKeyFrames.size();
  for (KF* k : lFixedCameras) add_kf(k, true);
  std::vector<MP*> mps(lLocalMapPoints.begin(), lLocalMapPoints.end());
  std::vector<float> mpPos, eObs, eInv;
  std::vector<int> eKF, eMP;
  std::vector<uint8_t> eRight;
  std::vector<std::pair<KF*, MP*>> eOwner;
  for (int j = 0; j < (int)mps.size(); ++j) {
    MP* pMP = mps[j];
    const auto X = pMP->GetWorldPos();
    mpPos.push_back(X(0)); mpPos.push_back(X(1)); mpPos.push_back(X(2));
    for (const auto& ob : pMP->GetObservations()) {
      KF* pKFi = ob.first;
      if (pKFi->isBad() || pKFi->GetMap() != pCurrentMap) continue;
      const auto it = kfIndex.find(pKFi);
      if (it == kfIndex.end()) continue;   // (a keyframe g2o has no vertex for: optimizer.vertex(id) would be NULL)
      const int leftIndex = std::get<0>(ob.second);
      if (leftIndex != -1) {               // :1236-1290: monocular (mvuRight < 0) or stereo observation of the left camera
        const auto& kp = pKFi->NLeft == -1 ? pKFi->mvKeysUn[leftIndex] : pKFi->mvKeys[leftIndex];
        eKF.push_back(it->second); eMP.push_back(j); eRight.push_back(0);
        eObs.push_back(kp.pt.x); eObs.push_back(kp.pt.y); eObs.push_back(pKFi->mvuRight[leftIndex]);
        eInv.push_back(pKFi->mvInvLevelSigma2[kp.octave]);
        eOwner.emplace_back(pKFi, pMP);
      }
      if (pKFi->mpCamera2) {               // :1292-1330: EdgeSE3ProjectXYZToBody on the right camera
        const int rightIndex = std::get<1>(ob.second);
        if (rightIndex != -1) {
          const auto& kp = pKFi->mvKeysRight[rightIndex - pKFi->NLeft];
          eKF.push_back(it->second); eMP.push_back(j); eRight.push_back(1);
          eObs.push_back(kp.pt.x); eObs.push_back(kp.pt.y); eObs.push_back(-1.f);
          eInv.push_back(pKFi->mvInvLevelSigma2[kp.octave]);
          eOwner.emplace_back(pKFi, pMP);
        }
      }
    }
  }
  num_MPs = (int)mps.size();
  num_edges = (int)eKF.size();
  if (pbStopFlag && *pbStopFlag) return;   // :1353-1354
  LocalBAView g;
  g.nKF = (int)kfs.size(); g.nMP = (int)mps.size(); g.nE = (int)eKF.size();
  g.kfPose = kfPose.data(); g.kfFixed = kfFixed.data(); g.mpPos = mpPos.data(); g.eKF = eKF.data(); g.eMP = eMP.data();
  g.eObs = eObs.data(); g.eInvSigma2 = eInv.data();
  g.fx = pKF->fx; g.fy = pKF->fy; g.cx = pKF->cx; g.cy = pKF->cy; g.mbf = pKF->mbf;
  g.inertialMap = pMap->IsInertial();   // :1137
  float rigp[28];
  if (rig) { morb_glue::rig28(pKF, rigp); g.rig28 = rigp; g.eRight = eRight.data(); }
  LocalBundleAdjustment(g, pbStopFlag);
  // :1366-1401: the library marks the observations the reference erases (chi2 > 5.991 / 7.815 or non-positive depth); bad points are skipped here
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);   // :1404
  for (size_t e = 0; e < eOwner.size(); ++e)
    if (g.eraseFlag[e] && !eOwner[e].second->isBad()) {
      eOwner[e].first->EraseMapPointMatch(eOwner[e].second);
      eOwner[e].second->EraseObservation(eOwner[e].first);
    }
  int i = 0;
  for (KF* k : lLocalKeyFrames) k->SetPose(morb_glue::make_se3<SE3>(&kfPose[(size_t)7 * i++]));   // :1416-1425
  for (int j = 0; j < (int)mps.size(); ++j) {   // :1428-1436
    typename std::decay<decltype(mps[j]->GetWorldPos())>::type X;
    for (int k = 0; k < 3; ++k) X(k) = mpPos[3 * j + k];
    mps[j]->SetWorldPos(X);
    mps[j]->UpdateNormalAndDepth();
  }
  pMap->IncreaseChangeIndex();
}

// void Optimizer::LocalInertialBA(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int&, int&, int&, int&, bool bLarge, bool bRecInit)  Optimizer.cc:2324-2897
template <class KF, class MapT>
void Optimizer::LocalInertialBA(KF* pKF, bool* pbStopFlag, MapT* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs, int& num_edges, bool bLarge,
                                bool bRecInit) {
  using SE3 = typename std::decay<decltype(pKF->GetPose())>::type;
  using MP = typename std::remove_pointer<typename std::decay<decltype(pKF->GetMapPointMatches()[0])>::type>::type;
  using Bias = typename std::decay<decltype(pKF->GetImuBias())>::type;
  MapT* pCurrentMap = pKF->GetMap();
  const int maxOpt = bLarge ? 25 : 10;                                                // :2330-2335
  const int Nd = std::min((int)pCurrentMap->KeyFramesInMap() - 2, maxOpt);
  // :2339-2352: the temporal window
  std::vector<KF*> vpOptimizableKFs;
  vpOptimizableKFs.reserve(Nd > 0 ? Nd : 1);
  vpOptimizableKFs.push_back(pKF);
  pKF->mnBALocalForKF = pKF->mnId;
  for (int i = 1; i < Nd; i++) {
    if (vpOptimizableKFs.back()->mPrevKF) {
      vpOptimizableKFs.push_back(vpOptimizableKFs.back()->mPrevKF);
      vpOptimizableKFs.back()->mnBALocalForKF = pKF->mnId;
    } else break;
  }
  int N = (int)vpOptimizableKFs.size();
  std::list<MP*> lLocalMapPoints;                                                       // :2357-2371
  for (int i = 0; i < N; i++)
    for (MP* pMP : vpOptimizableKFs[i]->GetMapPointMatches())
      if (pMP && !pMP->isBad() && pMP->mnBALocalForKF != pKF->mnId) { lLocalMapPoints.push_back(pMP); pMP->mnBALocalForKF = pKF->mnId; }
  std::list<KF*> lFixedKeyFrames;                                                       // :2374-2383
  if (vpOptimizableKFs.back()->mPrevKF) {
    lFixedKeyFrames.push_back(vpOptimizableKFs.back()->mPrevKF);
    vpOptimizableKFs.back()->mPrevKF->mnBAFixedForKF = pKF->mnId;
  } else {
    vpOptimizableKFs.back()->mnBALocalForKF = 0;
    vpOptimizableKFs.back()->mnBAFixedForKF = pKF->mnId;
    lFixedKeyFrames.push_back(vpOptimizableKFs.back());
    vpOptimizableKFs.pop_back();
  }
  // (:2386-2410: maxCovKF = 0 — no optimizable visual keyframes)
  const int maxFixKF = 200;                                                             // :2413-2435
  for (MP* pMP : lLocalMapPoints) {
    for (const auto& ob : pMP->GetObservations()) {
      KF* pKFi = ob.first;
      if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
        pKFi->mnBAFixedForKF = pKF->mnId;
        if (!pKFi->isBad()) { lFixedKeyFrames.push_back(pKFi); break; }
      }
    }
    if ((int)lFixedKeyFrames.size() >= maxFixKF) break;
  }
  // vertices (:2461-2521): temporal keyframes (kind 0), then the fixed ones: the first is the keyframe before the window (kind 1), the rest kind 2
  N = (int)vpOptimizableKFs.size();
  std::map<KF*, int> kfIndex;
  std::vector<KF*> kfs;
  std::vector<float> kfState;
  std::vector<uint8_t> kfKind;
  auto add_kf = [&](KF* k, int kind) {
    kfIndex[k] = (int)kfs.size(); kfs.push_back(k);
    float s[21];
    morb_glue::imu_state21(k, s); morb_glue::bias6(k->GetImuBias(), s + 15);
    kfState.insert(kfState.end(), s, s + 21);
    kfKind.push_back((uint8_t)kind);
  };
  for (KF* k : vpOptimizableKFs) add_kf(k, 0);
  { bool first = true; for (KF* k : lFixedKeyFrames) { add_kf(k, first && k->bImu ? 1 : 2); first = false; } }
  // inertial links (:2524-2601)
  std::vector<int> iKF1, iKF2;
  std::vector<morb_imu_preintegrated> iPre;
  std::vector<uint8_t> iRobust;
  std::vector<float> iInfoScale;
  for (int i = 0; i < N; i++) {
    KF* pKFi = vpOptimizableKFs[i];
    if (!pKFi->mPrevKF) continue;
    if (!(pKFi->bImu && pKFi->mPrevKF->bImu && pKFi->mpImuPreintegrated)) continue;
    pKFi->mpImuPreintegrated->SetNewBias(pKFi->mPrevKF->GetImuBias());                // :2533 (before the vertices are looked up, as the reference does)
    const auto a = kfIndex.find(pKFi->mPrevKF);
    if (a == kfIndex.end()) continue;                                                 // (:2547-2552: a vertex is missing)
    iKF1.push_back(a->second); iKF2.push_back(kfIndex[pKFi]);
    iPre.emplace_back(); morb_glue::fill_pre(iPre.back(), pKFi->mpImuPreintegrated);
    iRobust.push_back((i == N - 1 || bRecInit) ? 1 : 0);                              // :2563-2573
    iInfoScale.push_back(i == N - 1 ? 1e-2f : 1.f);
  }
  // points and visual edges (:2643-2762)
  const bool rig = pKF->mpCamera2 != nullptr;
  std::vector<MP*> mps(lLocalMapPoints.begin(), lLocalMapPoints.end());
  std::vector<float> mpPos, eObs, eInv;
  std::vector<uint8_t> mpClose, eRight;
  std::vector<int> eKF, eMP;
  std::vector<std::pair<KF*, MP*>> eOwner;
  for (int j = 0; j < (int)mps.size(); ++j) {
    MP* pMP = mps[j];
    const auto X = pMP->GetWorldPos();
    mpPos.push_back(X(0)); mpPos.push_back(X(1)); mpPos.push_back(X(2));
    mpClose.push_back(pMP->mTrackDepth < 10.f ? 1 : 0);                               // :2781
    for (const auto& ob : pMP->GetObservations()) {
      KF* pKFi = ob.first;
      if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) continue;
      if (pKFi->isBad() || pKFi->GetMap() != pCurrentMap) continue;
      const auto it = kfIndex.find(pKFi);
      if (it == kfIndex.end()) continue;
      const int leftIndex = std::get<0>(ob.second);
      if (leftIndex != -1) {                                                          // :2666-2722: EdgeMono(0) / EdgeStereo(0)
        const auto& kp = pKFi->mvKeysUn[leftIndex];
        eKF.push_back(it->second); eMP.push_back(j); eRight.push_back(0);
        eObs.push_back(kp.pt.x); eObs.push_back(kp.pt.y); eObs.push_back(pKFi->mvuRight[leftIndex]);
        eInv.push_back(pKFi->mvInvLevelSigma2[kp.octave]);
        eOwner.emplace_back(pKFi, pMP);
      }
      if (pKFi->mpCamera2) {                                                          // :2725-2758: EdgeMono(1) on the right camera
        const int rightIndex = std::get<1>(ob.second);
        if (rightIndex != -1) {
          const auto& kp = pKFi->mvKeysRight[rightIndex - pKFi->NLeft];
          eKF.push_back(it->second); eMP.push_back(j); eRight.push_back(1);
          eObs.push_back(kp.pt.x); eObs.push_back(kp.pt.y); eObs.push_back(-1.f);
          eInv.push_back(pKFi->mvInvLevelSigma2[kp.octave]);
          eOwner.emplace_back(pKFi, pMP);
        }
      }
    }
  }
  num_fixedKF = (int)lFixedKeyFrames.size(); num_OptKF = N; num_MPs = (int)mps.size(); num_edges = (int)eKF.size();
  LocalInertialBAView g;
  g.nKF = (int)kfs.size(); g.kfState = kfState.data(); g.kfKind = kfKind.data();
  g.nMP = (int)mps.size(); g.mpPos = mpPos.data(); g.mpClose = mpClose.data();
  g.nE = (int)eKF.size(); g.eKF = eKF.data(); g.eMP = eMP.data(); g.eObs = eObs.data(); g.eInvSigma2 = eInv.data();
  g.nI = (int)iKF1.size(); g.iKF1 = iKF1.data(); g.iKF2 = iKF2.data(); g.iPre = iPre.data(); g.iRobust = iRobust.data(); g.iInfoScale = iInfoScale.data();
  g.fx = pKF->fx; g.fy = pKF->fy; g.cx = pKF->cx; g.cy = pKF->cy; g.mbf = pKF->mbf;
  morb_glue::tbc12(pKF->mImuCalib.mTbc, g.Tbc12);
  float rigp[28];
  if (rig) { morb_glue::rig28(pKF, rigp); g.rig28 = rigp; g.eRight = eRight.data(); }
  g.bLarge = bLarge;
  LocalInertialBA(g);
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                             // :2808
  if (!g.ok) return;                                                                    // :2811-2815 "FAIL LOCAL-INERTIAL BA"
  for (size_t e = 0; e < eOwner.size(); ++e)                                            // :2773-2826
    if (g.eraseFlag[e] && !eOwner[e].second->isBad()) {
      eOwner[e].first->EraseMapPointMatch(eOwner[e].second);
      eOwner[e].second->EraseObservation(eOwner[e].first);
    }
  for (KF* k : lFixedKeyFrames) k->mnBAFixedForKF = 0;                                  // :2828-2831
  // :2836-2858: Tcw = (Rcb Rwb^T, tcb - Rcb Rwb^T twb) (ImuCamPose, G2oTypes.cc:74-113), velocity, bias
  float Tbc[12];
  morb_glue::tbc12(pKF->mImuCalib.mTbc, Tbc);
  for (int i = 0; i < N; i++) {
    KF* pKFi = vpOptimizableKFs[i];
    const float* s = &kfState[(size_t)21 * i];
    double Rcw[9], tcw[3];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) { double a = 0; for (int k = 0; k < 3; ++k) a += (double)Tbc[3 * k + r] * s[3 * c + k]; Rcw[3 * r + c] = a; }   // Rcb Rwb^T, Rcb = Rbc^T
    }
    for (int r = 0; r < 3; ++r) {
      double a = 0;
      for (int k = 0; k < 3; ++k) a -= (double)Tbc[3 * k + r] * Tbc[9 + k];            // tcb = -Rbc^T tbc
      for (int c = 0; c < 3; ++c) a -= Rcw[3 * r + c] * s[9 + c];
      tcw[r] = a;
    }
    pKFi->SetPose(se3_from_matrix<SE3>(Rcw, tcw));
    pKFi->mnBALocalForKF = 0;
    if (pKFi->bImu) {
      typename std::decay<decltype(pKFi->GetVelocity())>::type vel;
      for (int k = 0; k < 3; ++k) vel(k) = s[12 + k];
      pKFi->SetVelocity(vel);
      pKFi->SetNewBias(Bias(s[18], s[19], s[20], s[15], s[16], s[17]));
    }
  }
  for (int j = 0; j < (int)mps.size(); ++j) {                                           // :2873-2881
    typename std::decay<decltype(mps[j]->GetWorldPos())>::type X;
    for (int k = 0; k < 3; ++k) X(k) = mpPos[3 * j + k];
    mps[j]->SetWorldPos(X);
    mps[j]->UpdateNormalAndDepth();
  }
  pMap->IncreaseChangeIndex();
}
// Sophus::SE3f(Matrix3f Rcw, Vector3f tcw) (:2840-2842)
// int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2,
//                             const bool bFixScale, Eigen::Matrix<double, 7, 7>& mAcumHessian, const bool bAllPoints)  Optimizer.cc:2065-2322
// Gathers what the edge loop (:2118-2231) reads, runs morb_optimize_sim3_batch, nulls the vpMatches1 entries the two inlier tests null,
// and writes g2oS12 back / zeroes mAcumHessian only when the reference reaches its end (the early return at :2272 leaves both).
// Uses only g2o::Sim3's rotation() / translation() / scale() and (Quaterniond, Vector3d, double) constructor, and Matrix::setZero().
// Camera kind: a KannalaBrandt8 camera has 8 parameters, a Pinhole 4.  On a KB8 rig keyframe the reference's mvKeysUn[i] is out of bounds
// for i >= NLeft: feature i's own row is read (mvKeysRight[i - NLeft]), as DESIGN.md section 6 decides for SearchByProjection(Frame, KeyFrame).
template <class KF, class MP, class Sim3T, class Mat77>
int Optimizer::OptimizeSim3(KF* pKF1, KF* pKF2, std::vector<MP*>& vpMatches1, Sim3T& g2oS12, const float th2, const bool bFixScale,
                            Mat77& mAcumHessian, const bool bAllPoints) {
  const int N = (int)vpMatches1.size();
  const std::vector<MP*> vpMapPoints1 = pKF1->GetMapPointMatches();
  std::vector<uint8_t> entry(N, 0);
  std::vector<float> Xw1((size_t)N * 3, 0.f), Xw2((size_t)N * 3, 0.f), obs1((size_t)N * 2, 0.f), obs2((size_t)N * 2, 0.f), inv1(N, 0.f), inv2(N, 0.f);
  std::vector<int> i2v(N, -1);
  auto key_of = [](KF* pKF, int i) -> decltype(pKF->mvKeysUn[0]) {
    return (pKF->NLeft != -1 && i >= pKF->NLeft) ? pKF->mvKeysRight[i - pKF->NLeft] : pKF->mvKeysUn[i];
  };
  for (int i = 0; i < N; ++i) {
    MP* pMP2 = vpMatches1[i];
    if (!pMP2) continue;
    MP* pMP1 = vpMapPoints1[i];
    uint8_t e = 1;
    const int i2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKF2));
    i2v[i] = i2;
    if (pMP1) {
      e |= 2;
      if (pMP1->isBad()) e |= 4;
      const auto X = pMP1->GetWorldPos();
      for (int k = 0; k < 3; ++k) Xw1[(size_t)i * 3 + k] = X(k);
    }
    if (pMP2->isBad()) e |= 8;
    const auto X2 = pMP2->GetWorldPos();
    for (int k = 0; k < 3; ++k) Xw2[(size_t)i * 3 + k] = X2(k);
    entry[i] = e;
    if (!(e & 2) || (e & 12)) continue;   // no edge: nothing else is read
    const auto& kp1 = key_of(pKF1, i);
    obs1[(size_t)i * 2] = kp1.pt.x; obs1[(size_t)i * 2 + 1] = kp1.pt.y;
    inv1[i] = pKF1->mvInvLevelSigma2[kp1.octave];
    if (i2 >= 0) {
      const auto& kp2 = key_of(pKF2, i2);
      obs2[(size_t)i * 2] = kp2.pt.x; obs2[(size_t)i * 2 + 1] = kp2.pt.y;
      inv2[i] = pKF2->mvInvLevelSigma2[kp2.octave];
    } else {
      // kpUn2 = cv::KeyPoint(cv::Point2f(x, y), pMP2->mnTrackScaleLevel): that argument is the keypoint's SIZE, its octave stays 0
      inv2[i] = pKF2->mvInvLevelSigma2[0];
    }
  }
  OptimizeSim3View v;
  v.N = N; v.entry = entry.data(); v.Xw1 = Xw1.data(); v.Xw2 = Xw2.data(); v.i2 = i2v.data();
  v.obs1 = obs1.data(); v.invSigma2_1 = inv1.data(); v.obs2 = obs2.data(); v.invSigma2_2 = inv2.data();
  auto pose12 = [](KF* pKF, float* T) {
    const auto Tcw = pKF->GetPose();
    const auto R = Tcw.rotationMatrix();
    const auto t = Tcw.translation();
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) T[r * 3 + c] = R(r, c);
    for (int k = 0; k < 3; ++k) T[9 + k] = t(k);
  };
  pose12(pKF1, v.T1w); pose12(pKF2, v.T2w);
  auto cam9 = [](KF* pKF, float* c) {
    morb_glue::cam8(pKF->mpCamera, c + 1);
    c[0] = pKF->mpCamera->size() >= 8 ? 1.f : 0.f;
  };
  cam9(pKF1, v.cam1); cam9(pKF2, v.cam2);
  v.th2 = th2; v.bFixScale = bFixScale; v.bAllPoints = bAllPoints;
  const auto& q = g2oS12.rotation();
  v.S12[0] = q.x(); v.S12[1] = q.y(); v.S12[2] = q.z(); v.S12[3] = q.w();
  for (int k = 0; k < 3; ++k) v.S12[4 + k] = g2oS12.translation()(k);
  v.S12[7] = g2oS12.scale();
  const int nIn = OptimizeSim3(v);
  for (int i = 0; i < N; ++i)
    if (vpMatches1[i] && !v.keep[i]) vpMatches1[i] = static_cast<MP*>(NULL);
  if (v.stats[4]) {
    using Quat = typename std::decay<decltype(g2oS12.rotation())>::type;
    using Vec3 = typename std::decay<decltype(g2oS12.translation())>::type;
    Vec3 t;
    for (int k = 0; k < 3; ++k) t(k) = v.S12[4 + k];
    g2oS12 = Sim3T(Quat(v.S12[3], v.S12[0], v.S12[1], v.S12[2]), t, v.S12[7]);
    mAcumHessian.setZero();
  }
  return nIn;
}

// Optimizer::OptimizeEssentialGraph, overload 1 (Optimizer.cc:1443-1735), flattened for morb_optimize_essential_graph.  Vertices: the keyframes of
// GetAllKeyFrames() that are not bad, in ascending mnId (the order of elimination); estimate = CorrectedSim3's entry or the pose with s = 1
// (:1485-1495), fixed = the map's initial keyframe (:1497), _fix_scale = bFixScale (:1501).  Edges in the reference's insertion order and
// under its conditions (:1514-1682); an edge whose endpoint has no vertex (a bad keyframe) is dropped, as g2o's addEdge drops it — its pair
// still enters sInsertedEdges (:1548).  Points in GetAllMapPoints() order, mpRef = -1 for a bad one.
struct EssentialGraphFlat {
  std::vector<double> kfSim3, eSji;
  std::vector<uint8_t> kfFlags;
  std::vector<int> eI, eJ, mpRef;
  std::vector<float> mpPos;
  std::map<unsigned long, int> row;   // mnId -> vertex
};
namespace morb_glue {
template <class S> inline void sim3_to8(const S& g, double* o) {
  const auto q = g.rotation();
  o[0] = q.x(); o[1] = q.y(); o[2] = q.z(); o[3] = q.w();
  for (int k = 0; k < 3; ++k) o[4 + k] = g.translation()(k);
  o[7] = g.scale();
}
template <class MapT, class KF, class CorrMap, class ConnMap>
void flatten_essential_graph(MapT* pMap, KF* pLoopKF, KF* pCurKF, const CorrMap& NonCorrectedSim3, const CorrMap& CorrectedSim3, const ConnMap& LoopConnections,
                             bool bFixScale, EssentialGraphFlat& f) {
  using Sim3T = typename CorrMap::mapped_type;
  using Quat = typename std::decay<decltype(std::declval<Sim3T>().rotation())>::type;
  using Vec3 = typename std::decay<decltype(std::declval<Sim3T>().translation())>::type;
  const auto vpKFs = pMap->GetAllKeyFrames();
  const auto vpMPs = pMap->GetAllMapPoints();
  const int minFeat = 100;
  for (KF* pKF : vpKFs) if (!pKF->isBad()) f.row[pKF->mnId] = 0;
  int n = 0;
  for (auto& kv : f.row) kv.second = n++;
  std::vector<Sim3T> vScw(n);
  f.kfSim3.assign((size_t)n * 8, 0.0); f.kfFlags.assign(n, 0);
  for (KF* pKF : vpKFs) {   // :1478-1507
    if (pKF->isBad()) continue;
    const int r = f.row[pKF->mnId];
    const auto it = CorrectedSim3.find(pKF);
    if (it != CorrectedSim3.end()) vScw[r] = it->second;
    else {   // Sophus::SE3d Tcw = pKF->GetPose().cast<double>(); g2o::Sim3 Siw(Tcw.unit_quaternion(), Tcw.translation(), 1.0)
      const auto Tcw = pKF->GetPose();
      const auto q = Tcw.unit_quaternion();
      const auto t = Tcw.translation();
      Vec3 td;
      for (int k = 0; k < 3; ++k) td(k) = (double)t(k);
      vScw[r] = Sim3T(Quat((double)q.w(), (double)q.x(), (double)q.y(), (double)q.z()), td, 1.0);
    }
    sim3_to8(vScw[r], &f.kfSim3[(size_t)r * 8]);
    f.kfFlags[r] = (pKF->mnId == pMap->GetInitKFid() ? 1 : 0) | (bFixScale ? 2 : 0);
  }
  auto rowOf = [&](unsigned long id) { const auto it = f.row.find(id); return it == f.row.end() ? -1 : it->second; };
  auto add = [&](unsigned long idi, unsigned long idj, const Sim3T& Sji) {   // setVertex(0, i), setVertex(1, j); addEdge refuses a missing vertex
    const int ri = rowOf(idi), rj = rowOf(idj);
    if (ri < 0 || rj < 0) return;
    f.eI.push_back(ri); f.eJ.push_back(rj);
    f.eSji.resize(f.eSji.size() + 8);
    sim3_to8(Sji, &f.eSji[f.eSji.size() - 8]);
  };
  auto nonCorrected = [&](KF* pKF, Sim3T& out) {   // NonCorrectedSim3's entry, else vScw (false: the keyframe has neither)
    const auto it = NonCorrectedSim3.find(pKF);
    if (it != NonCorrectedSim3.end()) { out = it->second; return true; }
    const int r = rowOf(pKF->mnId);
    if (r < 0) return false;
    out = vScw[r];
    return true;
  };
  std::set<std::pair<unsigned long, unsigned long>> sInsertedEdges;
  for (auto mit = LoopConnections.begin(); mit != LoopConnections.end(); ++mit) {   // :1516-1550
    KF* pKF = mit->first;
    const unsigned long nIDi = pKF->mnId;
    const int ri = rowOf(nIDi);
    for (auto sit = mit->second.begin(); sit != mit->second.end(); ++sit) {
      const unsigned long nIDj = (*sit)->mnId;
      if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
      const int rj = rowOf(nIDj);
      if (ri >= 0 && rj >= 0) add(nIDi, nIDj, vScw[rj] * vScw[ri].inverse());
      sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
    }
  }
  for (KF* pKF : vpKFs) {   // :1553-1682
    if (rowOf(pKF->mnId) < 0) continue;   // (every edge below has this keyframe as vertex 0)
    Sim3T Siw;
    nonCorrected(pKF, Siw);
    const Sim3T Swi = Siw.inverse();
    KF* pParentKF = pKF->GetParent();
    Sim3T Sjw;
    if (pParentKF && nonCorrected(pParentKF, Sjw)) add(pKF->mnId, pParentKF->mnId, Sjw * Swi);
    const auto sLoopEdges = pKF->GetLoopEdges();
    for (auto sit = sLoopEdges.begin(); sit != sLoopEdges.end(); ++sit) {
      KF* pLKF = *sit;
      if (pLKF->mnId < pKF->mnId && nonCorrected(pLKF, Sjw)) add(pKF->mnId, pLKF->mnId, Sjw * Swi);
    }
    const auto vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
    for (auto vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); ++vit) {
      KF* pKFn = *vit;
      if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn)) {
        if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
          if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
          if (nonCorrected(pKFn, Sjw)) add(pKF->mnId, pKFn->mnId, Sjw * Swi);
        }
      }
    }
    if (pKF->bImu && pKF->mPrevKF) {
      KF* pPrev = static_cast<KF*>(pKF->mPrevKF);
      if (nonCorrected(pPrev, Sjw)) add(pKF->mnId, pPrev->mnId, Sjw * Swi);
    }
  }
  f.mpPos.assign(vpMPs.size() * 3, 0.f); f.mpRef.assign(vpMPs.size(), -1);
  for (size_t i = 0; i < vpMPs.size(); ++i) {   // :1709-1723
    auto* pMP = vpMPs[i];
    if (pMP->isBad()) continue;
    const unsigned long nIDr = pMP->mnCorrectedByKF == pCurKF->mnId ? (unsigned long)pMP->mnCorrectedReference : pMP->GetReferenceKeyFrame()->mnId;
    f.mpRef[i] = rowOf(nIDr);
    const auto X = pMP->GetWorldPos();
    for (int k = 0; k < 3; ++k) f.mpPos[i * 3 + k] = X(k);
  }
}
}  // namespace morb_glue

template <class MapT, class KF, class CorrMap, class ConnMap>
void Optimizer::OptimizeEssentialGraph(MapT* pMap, KF* pLoopKF, KF* pCurKF, const CorrMap& NonCorrectedSim3, const CorrMap& CorrectedSim3,
                                       const ConnMap& LoopConnections, const bool& bFixScale) {
  EssentialGraphFlat f;
  morb_glue::flatten_essential_graph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale, f);
  EssentialGraphView g;
  g.nKF = (int)f.kfFlags.size(); g.nE = (int)f.eI.size(); g.nMP = (int)f.mpRef.size();
  g.kfSim3 = f.kfSim3.data(); g.kfFlags = f.kfFlags.data(); g.eI = f.eI.data(); g.eJ = f.eJ.data(); g.eSji = f.eSji.data();
  g.mpPos = g.nMP ? f.mpPos.data() : nullptr; g.mpRef = g.nMP ? f.mpRef.data() : nullptr;
  if (g.nKF > 0) OptimizeEssentialGraph(g);   // optimize(20) (:1684-1687)
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);   // :1688
  const auto vpKFs = pMap->GetAllKeyFrames();
  for (KF* pKFi : vpKFs) {   // SE3 pose recovering, Sim3 [sR t; 0 1] -> SE3 [R t / s; 0 1] (:1691-1705)
    const auto it = f.row.find(pKFi->mnId);
    if (it == f.row.end()) continue;   // (a bad keyframe has no vertex)
    const double* S = &f.kfSim3[(size_t)it->second * 8];
    // Sophus::SE3f Tiw(rotation().cast<float>(), translation().cast<float>() / s): the float vector divided by the scale as a float
    const float s = (float)S[7];
    const float p7[7] = {(float)S[0], (float)S[1], (float)S[2], (float)S[3], (float)S[4] / s, (float)S[5] / s, (float)S[6] / s};
    pKFi->SetPose(morb_glue::make_se3<typename std::decay<decltype(pKFi->GetPose())>::type>(p7));
  }
  const auto vpMPs = pMap->GetAllMapPoints();
  for (size_t i = 0; i < vpMPs.size(); ++i) {   // :1709-1731
    auto* pMP = vpMPs[i];
    if (pMP->isBad()) continue;
    if (f.mpRef[i] >= 0) {
      typename std::decay<decltype(pMP->GetWorldPos())>::type X;
      for (int k = 0; k < 3; ++k) X(k) = f.mpPos[i * 3 + k];
      pMP->SetWorldPos(X);
    }
    pMP->UpdateNormalAndDepth();
  }
  pMap->IncreaseChangeIndex();   // :1734
}

// Optimizer::OptimizeEssentialGraph, overload 2 (Optimizer.cc:1737-2063), flattened for morb_optimize_essential_graph_merge.  Vertices: the
// keyframes of the three lists that are not bad, in ascending mnId, each with the lists it is in.  Candidate edges in the reference's insertion
// order (:1888-1999) — vpKFs is the three lists one behind the other, so a keyframe of two lists gives its candidates twice — with its
// hasChild, sLoopEdges.count and mnId < tests; a candidate whose end has no vertex (a bad keyframe is neither good nor bad, :1907-1913) is
// left out, the good / bad rule itself is the entry's.  Points in vpNonCorrectedMPs order: mpRef = the vertex of the reference keyframe behind
// the while (pRefKF->isBad()) EraseObservation loop of :2038-2048, -1 for a bad point and for a reference outside the lists.  Where the
// reference is undefined this skips: a point without a reference keyframe (:2038 dereferences it), an mnId beyond GetMaxKFid() (the
// reference's vectors have nMaxKFid + 1 entries).  A keyframe listed twice in vpNonFixedKFs gets the tail once.
struct MergeGraphFlat {
  std::vector<uint8_t> kfLists, cKept;
  std::vector<float> kfTcw, kfTwc, kfTcwBefMerge, kfTwcBefMerge, mpPos;
  std::vector<int> cI, cJ, mpRef;
  std::map<unsigned long, int> row;   // mnId -> vertex
};
namespace morb_glue {
template <class KF, class MP>
void flatten_merge_graph(KF* pCurKF, std::vector<KF*>& vpFixedKFs, std::vector<KF*>& vpFixedCorrectedKFs, std::vector<KF*>& vpNonFixedKFs,
                         std::vector<MP*>& vpNonCorrectedMPs, MergeGraphFlat& f) {
  auto* pMap = pCurKF->GetMap();
  const unsigned long nMaxKFid = pMap->GetMaxKFid();
  const int minFeat = 100;
  std::map<unsigned long, std::pair<KF*, int>> byId;   // mnId -> keyframe, lists
  std::vector<KF*>* const lists[3] = {&vpFixedKFs, &vpFixedCorrectedKFs, &vpNonFixedKFs};
  for (int l = 0; l < 3; ++l)
    for (KF* pKFi : *lists[l]) {
      if (pKFi->isBad() || pKFi->mnId > nMaxKFid) continue;
      auto& e = byId[pKFi->mnId];
      e.first = pKFi; e.second |= 1 << l;
    }
  const int n = (int)byId.size();
  f.kfLists.resize(n); f.kfTcw.resize((size_t)n * 7); f.kfTwc.resize((size_t)n * 7); f.kfTcwBefMerge.resize((size_t)n * 7); f.kfTwcBefMerge.resize((size_t)n * 7);
  int r = 0;
  for (auto& kv : byId) {
    KF* pKFi = kv.second.first;
    f.row[kv.first] = r;
    f.kfLists[r] = (uint8_t)kv.second.second;
    pose7(pKFi->GetPose(), &f.kfTcw[(size_t)r * 7]); pose7(pKFi->GetPoseInverse(), &f.kfTwc[(size_t)r * 7]);
    pose7(pKFi->mTcwBefMerge, &f.kfTcwBefMerge[(size_t)r * 7]); pose7(pKFi->mTwcBefMerge, &f.kfTwcBefMerge[(size_t)r * 7]);
    ++r;
  }
  auto rowOf = [&](KF* k) { const auto it = f.row.find(k->mnId); return (it == f.row.end() || byId[k->mnId].first != k) ? -1 : it->second; };
  std::vector<KF*> vpKFs;   // :1876-1883
  vpKFs.insert(vpKFs.end(), vpFixedKFs.begin(), vpFixedKFs.end());
  vpKFs.insert(vpKFs.end(), vpFixedCorrectedKFs.begin(), vpFixedCorrectedKFs.end());
  vpKFs.insert(vpKFs.end(), vpNonFixedKFs.begin(), vpNonFixedKFs.end());
  std::set<KF*> spKFs(vpKFs.begin(), vpKFs.end());
  auto add = [&](int ri, KF* pKFj) {
    const int rj = rowOf(pKFj);
    if (rj < 0) return;
    f.cI.push_back(ri); f.cJ.push_back(rj);
  };
  for (KF* pKFi : vpKFs) {   // :1888-1999
    const int ri = pKFi->isBad() ? -1 : rowOf(pKFi);
    if (ri < 0) continue;
    KF* pParentKFi = pKFi->GetParent();
    if (pParentKFi && spKFs.find(pParentKFi) != spKFs.end()) add(ri, pParentKFi);
    const auto sLoopEdges = pKFi->GetLoopEdges();
    for (auto sit = sLoopEdges.begin(); sit != sLoopEdges.end(); ++sit) {
      KF* pLKF = *sit;
      if (spKFs.find(pLKF) != spKFs.end() && pLKF->mnId < pKFi->mnId) add(ri, pLKF);
    }
    const auto vpConnectedKFs = pKFi->GetCovisiblesByWeight(minFeat);
    for (auto vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); ++vit) {
      KF* pKFn = *vit;
      if (pKFn && pKFn != pParentKFi && !pKFi->hasChild(pKFn) && !sLoopEdges.count(pKFn) && spKFs.find(pKFn) != spKFs.end()) {
        if (!pKFn->isBad() && pKFn->mnId < pKFi->mnId) add(ri, pKFn);
      }
    }
  }
  f.cKept.assign(f.cI.size(), 0);
  f.mpPos.assign(vpNonCorrectedMPs.size() * 3, 0.f); f.mpRef.assign(vpNonCorrectedMPs.size(), -1);
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);   // (EraseObservation below is :2046's, which the reference runs under this lock)
  for (size_t i = 0; i < vpNonCorrectedMPs.size(); ++i) {   // :2034-2048
    MP* pMPi = vpNonCorrectedMPs[i];
    if (pMPi->isBad()) continue;
    KF* pRefKF = pMPi->GetReferenceKeyFrame();
    while (pRefKF && pRefKF->isBad()) {
      pMPi->EraseObservation(pRefKF);
      pRefKF = pMPi->GetReferenceKeyFrame();
    }
    if (!pRefKF || pRefKF->mnId > nMaxKFid) continue;
    f.mpRef[i] = rowOf(pRefKF);
    const auto X = pMPi->GetWorldPos();
    for (int k = 0; k < 3; ++k) f.mpPos[i * 3 + k] = X(k);
  }
}
}  // namespace morb_glue

template <class KF, class MP>
void Optimizer::OptimizeEssentialGraph(KF* pCurKF, std::vector<KF*>& vpFixedKFs, std::vector<KF*>& vpFixedCorrectedKFs, std::vector<KF*>& vpNonFixedKFs,
                                       std::vector<MP*>& vpNonCorrectedMPs) {
  MergeGraphFlat f;
  morb_glue::flatten_merge_graph(pCurKF, vpFixedKFs, vpFixedCorrectedKFs, vpNonFixedKFs, vpNonCorrectedMPs, f);
  MergeEssentialGraphView g;
  g.nKF = (int)f.kfLists.size(); g.nC = (int)f.cI.size(); g.nMP = (int)f.mpRef.size();
  g.kfLists = f.kfLists.data(); g.kfTcw = f.kfTcw.data(); g.kfTwc = f.kfTwc.data(); g.kfTcwBefMerge = f.kfTcwBefMerge.data(); g.kfTwcBefMerge = f.kfTwcBefMerge.data();
  g.cI = g.nC ? f.cI.data() : nullptr; g.cJ = g.nC ? f.cJ.data() : nullptr; g.cKept = g.nC ? f.cKept.data() : nullptr;
  g.mpPos = g.nMP ? f.mpPos.data() : nullptr; g.mpRef = g.nMP ? f.mpRef.data() : nullptr;
  if (g.nKF > 0) OptimizeEssentialGraph(g);   // optimize(20) (:2009-2010) and the tail's arithmetic
  auto* pMap = pCurKF->GetMap();
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);   // :2012
  std::set<unsigned long> done;
  for (KF* pKFi : vpNonFixedKFs) {   // :2015-2030
    if (pKFi->isBad()) continue;
    const auto it = f.row.find(pKFi->mnId);
    if (it == f.row.end() || !done.insert(pKFi->mnId).second) continue;
    pKFi->mTcwBefMerge = pKFi->GetPose();
    pKFi->mTwcBefMerge = pKFi->GetPoseInverse();
    pKFi->SetPose(morb_glue::make_se3<typename std::decay<decltype(pKFi->GetPose())>::type>(&f.kfTcw[(size_t)it->second * 7]));
  }
  for (size_t i = 0; i < vpNonCorrectedMPs.size(); ++i) {   // :2034-2062
    MP* pMPi = vpNonCorrectedMPs[i];
    if (pMPi->isBad() || f.mpRef[i] < 0 || !(f.kfLists[f.mpRef[i]] & 6)) continue;   // (:2059: a reference of vpFixedKFs, the point stays)
    typename std::decay<decltype(pMPi->GetWorldPos())>::type X;
    for (int k = 0; k < 3; ++k) X(k) = f.mpPos[i * 3 + k];
    pMPi->SetWorldPos(X);
    pMPi->UpdateNormalAndDepth();
  }
}

// Optimizer::OptimizeEssentialGraph4DoF (Optimizer.cc:5163-5472), flattened for morb_optimize_essential_graph_4dof.  Vertices: the keyframes
// of GetAllKeyFrames() that are not bad, in ascending mnId; VertexPose4DoF(pKF) from the keyframe's float members, or
// VertexPose4DoF(Rwc, twc, pKF) from CorrectedSim3's inverse (:5201-5214); fixed = pLoopKF (:5216).  mImuCalib.mTcb is taken from the first
// keyframe with a vertex: one calibration per map.  Edges in the reference's insertion order and under its conditions (:5236-5426); each
// measurement is the rotation and the translation of the Sim3 product.  Where the reference is undefined this skips: its normal-edge and
// write-back loops do not test isBad(), and mPrevKF or a loop connection may name a keyframe without a vertex (optimizer.vertex() is NULL
// there) — an edge with such an endpoint is dropped (its pair still enters sInsertedEdges), a keyframe without a vertex contributes no
// edges of its own and keeps its pose, and a point whose reference keyframe has no vertex keeps its position.
struct PoseGraph4DoFFlat {
  std::vector<double> kfPose, kfBody, kfScw, eTij;
  std::vector<uint8_t> kfFixed;
  std::vector<int> eI, eJ, mpRef;
  std::vector<float> mpPos;
  float Tcb12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  std::map<unsigned long, int> row;   // mnId -> vertex
};
namespace morb_glue {
template <class Q> inline void quat_to_matrix(const Q& q, double* R) {   // Eigen::QuaternionBase::toRotationMatrix
  const double x = q.x(), y = q.y(), z = q.z(), w = q.w();
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
inline void matrix_to_quat(const double* m, double* q) {   // Eigen::Quaterniond(Matrix3d): x y z w
  double t = m[0] + m[4] + m[8];
  if (t > 0) {
    t = std::sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t;
    q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
    q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
  }
}
template <class MapT, class KF, class CorrMap, class ConnMap>
void flatten_pose_graph_4dof(MapT* pMap, KF* pLoopKF, KF* pCurKF, const CorrMap& NonCorrectedSim3, const CorrMap& CorrectedSim3, const ConnMap& LoopConnections,
                             PoseGraph4DoFFlat& f) {
  using Sim3T = typename CorrMap::mapped_type;
  using Quat = typename std::decay<decltype(std::declval<Sim3T>().rotation())>::type;
  using Vec3 = typename std::decay<decltype(std::declval<Sim3T>().translation())>::type;
  const auto vpKFs = pMap->GetAllKeyFrames();
  const auto vpMPs = pMap->GetAllMapPoints();
  const int minFeat = 100;
  for (KF* pKF : vpKFs) if (!pKF->isBad()) f.row[pKF->mnId] = 0;
  int n = 0;
  for (auto& kv : f.row) kv.second = n++;
  std::vector<Sim3T> vScw(n);
  f.kfPose.assign((size_t)n * 12, 0.0); f.kfBody.assign((size_t)n * 12, 0.0); f.kfScw.assign((size_t)n * 8, 0.0); f.kfFixed.assign(n, 0);
  bool haveCalib = false;
  double Rcb[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tcb[3] = {0, 0, 0};
  for (KF* pKF : vpKFs) {   // :5194-5224
    if (pKF->isBad()) continue;
    if (!haveCalib) {
      const auto R = pKF->mImuCalib.mTcb.rotationMatrix();
      const auto t = pKF->mImuCalib.mTcb.translation();
      for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) f.Tcb12[r * 3 + c] = R(r, c); f.Tcb12[9 + r] = t(r); }
      for (int k = 0; k < 9; ++k) Rcb[k] = (double)f.Tcb12[k];
      for (int k = 0; k < 3; ++k) tcb[k] = (double)f.Tcb12[9 + k];
      haveCalib = true;
    }
    const int r = f.row[pKF->mnId];
    double* P = &f.kfPose[(size_t)r * 12];
    double* B = &f.kfBody[(size_t)r * 12];
    const auto it = CorrectedSim3.find(pKF);
    if (it != CorrectedSim3.end()) {   // VertexPose4DoF(Rwc, twc, pKF): G2oTypes.cc:120-146
      vScw[r] = it->second;
      const Sim3T Swc = it->second.inverse();
      double Rwc[9], twc[3];
      quat_to_matrix(Swc.rotation(), Rwc);
      for (int k = 0; k < 3; ++k) twc[k] = Swc.translation()(k);
      for (int a = 0; a < 3; ++a) {
        B[9 + a] = Rwc[a * 3] * tcb[0] + Rwc[a * 3 + 1] * tcb[1] + Rwc[a * 3 + 2] * tcb[2] + twc[a];
        for (int c = 0; c < 3; ++c) {
          B[a * 3 + c] = Rwc[a * 3] * Rcb[c] + Rwc[a * 3 + 1] * Rcb[3 + c] + Rwc[a * 3 + 2] * Rcb[6 + c];
          P[a * 3 + c] = Rwc[c * 3 + a];
        }
      }
      for (int a = 0; a < 3; ++a) P[9 + a] = -(P[a * 3] * twc[0] + P[a * 3 + 1] * twc[1] + P[a * 3 + 2] * twc[2]);
    } else {   // VertexPose4DoF(pKF): the float members, cast
      const auto Tcw = pKF->GetPose();
      const auto q = Tcw.unit_quaternion();
      const auto t = Tcw.translation();
      Vec3 td;
      for (int k = 0; k < 3; ++k) td(k) = (double)t(k);
      vScw[r] = Sim3T(Quat((double)q.w(), (double)q.x(), (double)q.y(), (double)q.z()), td, 1.0);
      const auto Rcw = pKF->GetRotation();
      const auto tcw = pKF->GetTranslation();
      const auto Rwb = pKF->GetImuRotation();
      const auto twb = pKF->GetImuPosition();
      for (int a = 0; a < 3; ++a) {
        for (int c = 0; c < 3; ++c) { P[a * 3 + c] = (double)Rcw(a, c); B[a * 3 + c] = (double)Rwb(a, c); }
        P[9 + a] = (double)tcw(a); B[9 + a] = (double)twb(a);
      }
    }
    sim3_to8(vScw[r], &f.kfScw[(size_t)r * 8]);
    f.kfFixed[r] = pKF == pLoopKF ? 1 : 0;
  }
  auto rowOf = [&](unsigned long id) { const auto it = f.row.find(id); return it == f.row.end() ? -1 : it->second; };
  auto add = [&](unsigned long idi, unsigned long idj, const Sim3T& Sij) {   // setVertex(0, i), setVertex(1, j)
    const int ri = rowOf(idi), rj = rowOf(idj);
    if (ri < 0 || rj < 0) return;
    f.eI.push_back(ri); f.eJ.push_back(rj);
    f.eTij.resize(f.eTij.size() + 12);
    double* T = &f.eTij[f.eTij.size() - 12];
    quat_to_matrix(Sij.rotation(), T);
    for (int k = 0; k < 3; ++k) T[9 + k] = Sij.translation()(k);
  };
  auto nonCorrected = [&](KF* pKF, Sim3T& out) {   // NonCorrectedSim3's entry, else vScw (false: the keyframe has neither)
    const auto it = NonCorrectedSim3.find(pKF);
    if (it != NonCorrectedSim3.end()) { out = it->second; return true; }
    const int r = rowOf(pKF->mnId);
    if (r < 0) return false;
    out = vScw[r];
    return true;
  };
  std::set<std::pair<unsigned long, unsigned long>> sInsertedEdges;
  for (auto mit = LoopConnections.begin(); mit != LoopConnections.end(); ++mit) {   // :5238-5274
    KF* pKF = mit->first;
    const unsigned long nIDi = pKF->mnId;
    const int ri = rowOf(nIDi);
    for (auto sit = mit->second.begin(); sit != mit->second.end(); ++sit) {
      const unsigned long nIDj = (*sit)->mnId;
      if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
      const int rj = rowOf(nIDj);
      if (ri >= 0 && rj >= 0) add(nIDi, nIDj, vScw[ri] * vScw[rj].inverse());
      sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
    }
  }
  for (KF* pKF : vpKFs) {   // :5277-5426 (pParentKF is NULL there: no spanning-tree edge)
    if (rowOf(pKF->mnId) < 0) continue;
    Sim3T Siw, Sjw;
    nonCorrected(pKF, Siw);
    KF* prevKF = static_cast<KF*>(pKF->mPrevKF);
    if (prevKF && nonCorrected(prevKF, Sjw)) add(pKF->mnId, prevKF->mnId, Siw * Sjw.inverse());
    const auto sLoopEdges = pKF->GetLoopEdges();
    for (auto sit = sLoopEdges.begin(); sit != sLoopEdges.end(); ++sit) {
      KF* pLKF = *sit;
      if (pLKF->mnId < pKF->mnId && nonCorrected(pLKF, Sjw)) add(pKF->mnId, pLKF->mnId, Siw * Sjw.inverse());
    }
    const auto vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
    for (auto vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); ++vit) {
      KF* pKFn = *vit;
      if (pKFn && pKFn != prevKF && pKFn != pKF->mNextKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
        if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
          if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
          if (nonCorrected(pKFn, Sjw)) add(pKF->mnId, pKFn->mnId, Siw * Sjw.inverse());
        }
      }
    }
  }
  f.mpPos.assign(vpMPs.size() * 3, 0.f); f.mpRef.assign(vpMPs.size(), -1);
  for (size_t i = 0; i < vpMPs.size(); ++i) {   // :5451-5461
    auto* pMP = vpMPs[i];
    if (pMP->isBad()) continue;
    f.mpRef[i] = rowOf(pMP->GetReferenceKeyFrame()->mnId);
    const auto X = pMP->GetWorldPos();
    for (int k = 0; k < 3; ++k) f.mpPos[i * 3 + k] = X(k);
  }
}
}  // namespace morb_glue

template <class MapT, class KF, class CorrMap, class ConnMap>
void Optimizer::OptimizeEssentialGraph4DoF(MapT* pMap, KF* pLoopKF, KF* pCurKF, const CorrMap& NonCorrectedSim3, const CorrMap& CorrectedSim3,
                                           const ConnMap& LoopConnections) {
  PoseGraph4DoFFlat f;
  morb_glue::flatten_pose_graph_4dof(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, f);
  PoseGraph4DoFView g;
  g.nKF = (int)f.kfFixed.size(); g.nE = (int)f.eI.size(); g.nMP = (int)f.mpRef.size();
  g.kfPose = f.kfPose.data(); g.kfBody = f.kfBody.data(); g.kfFixed = f.kfFixed.data(); g.eI = f.eI.data(); g.eJ = f.eJ.data(); g.eTij = f.eTij.data();
  std::memcpy(g.Tcb12, f.Tcb12, sizeof g.Tcb12);
  g.mpPos = g.nMP ? f.mpPos.data() : nullptr; g.mpRef = g.nMP ? f.mpRef.data() : nullptr; g.kfScw = g.nMP ? f.kfScw.data() : nullptr;
  if (g.nKF > 0) OptimizeEssentialGraph4DoF(g);   // optimize(20) (:5428-5430)
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);   // :5432
  const auto vpKFs = pMap->GetAllKeyFrames();
  for (KF* pKFi : vpKFs) {   // :5435-5448: g2o::Sim3(Ri, ti, 1.) -> Sophus::SE3d -> float
    const auto it = f.row.find(pKFi->mnId);
    if (it == f.row.end()) continue;   // (a bad keyframe has no vertex)
    const double* P = &f.kfPose[(size_t)it->second * 12];
    double q[4];
    morb_glue::matrix_to_quat(P, q);
    const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float p7[7] = {(float)(q[0] / nq), (float)(q[1] / nq), (float)(q[2] / nq), (float)(q[3] / nq), (float)P[9], (float)P[10], (float)P[11]};
    pKFi->SetPose(morb_glue::make_se3<typename std::decay<decltype(pKFi->GetPose())>::type>(p7));
  }
  const auto vpMPs = pMap->GetAllMapPoints();
  for (size_t i = 0; i < vpMPs.size(); ++i) {   // :5451-5470
    auto* pMP = vpMPs[i];
    if (pMP->isBad()) continue;
    if (f.mpRef[i] >= 0) {
      typename std::decay<decltype(pMP->GetWorldPos())>::type X;
      for (int k = 0; k < 3; ++k) X(k) = f.mpPos[i * 3 + k];
      pMP->SetWorldPos(X);
    }
    pMP->UpdateNormalAndDepth();
  }
  pMap->IncreaseChangeIndex();   // :5471
}

// The three Optimizer::InertialOptimization overloads (Optimizer.cc:2979-3428) around one flattening: GetAllKeyFrames() without the keyframes
// beyond GetMaxKFid() (:3007, :3191, :3339), ordered by walking the mPrevKF chains so that every link joins neighbours (a keyframe without a
// link starts a chain, in GetAllKeyFrames() order); a link under the conditions of :3077-3078 (mPrevKF set, not isBad(), mPrevKF not beyond
// maxKFid, its vertex present); vpKFs.front()'s bias as the initial bias.  fill sets what the overload passes in, back hands its by-reference
// results out.  Modes 0 and 1 then write SetVelocity / SetNewBias on every keyframe and Reintegrate() where flagged (:3131-3155, :3292-3313).
template <class MapT, class Fill, class Back>
void Optimizer::inertial_optimization_on_map(MapT* pMap, int mode, Fill fill, Back back) {
  const long unsigned int maxKFid = pMap->GetMaxKFid();
  const auto vpKFs = pMap->GetAllKeyFrames();
  if (vpKFs.empty()) return;
  using KF = typename std::remove_pointer<typename std::decay<decltype(vpKFs[0])>::type>::type;
  using Bias = typename std::decay<decltype(vpKFs[0]->GetImuBias())>::type;
  std::vector<KF*> kept;
  std::map<KF*, int> index;
  for (KF* k : vpKFs)
    if (k->mnId <= maxKFid) { index[k] = (int)kept.size(); kept.push_back(k); }
  const int n = (int)kept.size();
  std::vector<int> pred(n, -1), succ(n, -1);
  for (int i = 0; i < n; ++i) {
    KF* k = kept[i];
    if (!k->mPrevKF) continue;
    if (k->isBad() || k->mPrevKF->mnId > maxKFid) continue;
    if (!k->mpImuPreintegrated) continue;                                            // ("Not preintegrated measurement", :3079-3080)
    if (mode != 2) k->mpImuPreintegrated->SetNewBias(k->mPrevKF->GetImuBias());       // :3082, :3263
    const auto a = index.find(k->mPrevKF);
    if (a == index.end() || succ[a->second] >= 0) continue;                           // (a vertex is missing; mPrevKF chains do not branch)
    pred[i] = a->second; succ[a->second] = i;
  }
  std::vector<KF*> order;
  std::vector<uint8_t> hasLink;
  for (int i = 0; i < n; ++i) {
    if (pred[i] >= 0) continue;
    for (int j = i; j >= 0; j = succ[j]) { order.push_back(kept[j]); hasLink.push_back(j == i ? 0 : 1); }
  }
  std::vector<float> kfState((size_t)21 * n);
  std::vector<morb_imu_preintegrated> pre(n);
  for (int i = 0; i < n; ++i) {
    morb_glue::imu_state21(order[i], &kfState[(size_t)21 * i]);
    morb_glue::bias6(order[i]->GetImuBias(), &kfState[(size_t)21 * i + 15]);
    if (hasLink[i]) morb_glue::fill_pre(pre[i], order[i]->mpImuPreintegrated);
  }
  InertialOptimizationView v;
  v.nKF = n; v.kfState = kfState.data(); v.hasLink = hasLink.data(); v.pre = pre.data();
  { float b6[6]; morb_glue::bias6(vpKFs.front()->GetImuBias(), b6); for (int k = 0; k < 6; ++k) v.global16[10 + k] = b6[k]; }   // VertexGyroBias / VertexAccBias(vpKFs.front())
  fill(v);
  InertialOptimization(v, mode);
  if (!v.ok) return;
  back(v);
  if (mode == 2) return;
  for (int i = 0; i < n; ++i) {
    KF* k = order[i];
    const float* s = &kfState[(size_t)21 * i];
    typename std::decay<decltype(k->GetVelocity())>::type vel;
    for (int c = 0; c < 3; ++c) vel(c) = s[12 + c];
    k->SetVelocity(vel);
    k->SetNewBias(Bias(s[18], s[19], s[20], s[15], s[16], s[17]));
    if (v.reintegrate[i] && k->mpImuPreintegrated) k->mpImuPreintegrated->Reintegrate();
  }
}

// void Optimizer::InertialOptimization(Map* pMap, Eigen::Matrix3d& Rwg, double& scale, Eigen::Vector3d& bg, Eigen::Vector3d& ba, bool bMono,
//                                      Eigen::MatrixXd& covInertial, bool bFixedVel, bool bGauss, float priorG, float priorA)  Optimizer.cc:2979-3156
// (covInertial and bGauss are unused there and here)
template <class MapT, class Mat3d, class Vec3d, class MatXd>
void Optimizer::InertialOptimization(MapT* pMap, Mat3d& Rwg, double& scale, Vec3d& bg, Vec3d& ba, bool bMono, MatXd& /*covInertial*/, bool bFixedVel,
                                     bool /*bGauss*/, float priorG, float priorA) {
  inertial_optimization_on_map(
      pMap, 0,
      [&](InertialOptimizationView& v) {
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) v.global16[3 * r + c] = Rwg(r, c);
        v.global16[9] = scale; v.bMono = bMono; v.bFixedVel = bFixedVel; v.priorG = priorG; v.priorA = priorA;
      },
      [&](const InertialOptimizationView& v) {
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rwg(r, c) = v.global16[3 * r + c];
        scale = v.global16[9];
        for (int k = 0; k < 3; ++k) { bg(k) = v.global16[10 + k]; ba(k) = v.global16[13 + k]; }
      });
}
// void Optimizer::InertialOptimization(Map* pMap, Eigen::Vector3d& bg, Eigen::Vector3d& ba, float priorG, float priorA)  Optimizer.cc:3158-3314
template <class MapT, class Vec3d>
void Optimizer::InertialOptimization(MapT* pMap, Vec3d& bg, Vec3d& ba, float priorG, float priorA) {
  inertial_optimization_on_map(
      pMap, 1, [&](InertialOptimizationView& v) { v.priorG = priorG; v.priorA = priorA; },
      [&](const InertialOptimizationView& v) { for (int k = 0; k < 3; ++k) { bg(k) = v.global16[10 + k]; ba(k) = v.global16[13 + k]; } });
}
// void Optimizer::InertialOptimization(Map* pMap, Eigen::Matrix3d& Rwg, double& scale)  Optimizer.cc:3316-3428
template <class MapT, class Mat3d>
void Optimizer::InertialOptimization(MapT* pMap, Mat3d& Rwg, double& scale) {
  inertial_optimization_on_map(
      pMap, 2,
      [&](InertialOptimizationView& v) {
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) v.global16[3 * r + c] = Rwg(r, c);
        v.global16[9] = scale;
      },
      [&](const InertialOptimizationView& v) {
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rwg(r, c) = v.global16[3 * r + c];
        scale = v.global16[9];
      });
}

// void Optimizer::GlobalBundleAdjustemnt(Map* pMap, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust)  Optimizer.cc:47-54
template <class MapT>
void Optimizer::GlobalBundleAdjustemnt(MapT* pMap, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust) {
  const auto vpKFs = pMap->GetAllKeyFrames();
  const auto vpMP = pMap->GetAllMapPoints();
  BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust);
}
// void Optimizer::BundleAdjustment(const vector<KeyFrame*>& vpKFs, const vector<MapPoint*>& vpMP, int nIterations, bool* pbStopFlag, const unsigned long
//                                  nLoopKF, const bool bRobust)  Optimizer.cc:56-362, for the one map shape that is built: the map Tracking::
// CreateInitialMapMonocular has just made — two keyframes, the one with GetInitKFid() fixed (at the identity), every point observed by both
// through mono edges.  Flattened into an InitialMapView and solved with the scaling switched off (depthScale 0, minTracked 0); written back as
// :276-361 does for both nLoopKF cases (the `dist > 1` block of :297-340 only counts and is left out).  Any other map is refused with
// std::runtime_error, unless the integrator defines MORB_WHOLE_MAP_BUNDLE_ADJUSTMENT before including this header: then it goes to
// WholeMapBundleAdjustment below, and LoopClosing.cc:2302 compiles unchanged.  (The default keeps what tests/native/initial_map_member_check.cc pins.)
// false: the map is not the initial-map shape, *whyNot says why and nothing has been touched
template <class KF, class MP>
bool Optimizer::initial_map_bundle_adjustment(const std::vector<KF*>& vpKFs, const std::vector<MP*>& vpMP, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF,
                                              const bool bRobust, std::string* whyNot) {
  const char* what = "Optimizer::BundleAdjustment: only the map of a monocular initialisation is built (two keyframes, the initial one fixed at the identity, "
                     "every point seen by both through monocular observations); ";
  auto refuse = [&](const std::string& why) { *whyNot = std::string(what) + why; return false; };
  std::vector<KF*> kfs;
  for (KF* k : vpKFs) if (!k->isBad()) kfs.push_back(k);
  if (kfs.size() != 2) return refuse("this map has " + std::to_string(kfs.size()) + " keyframes");
  auto* pMap = vpKFs[0]->GetMap();
  const unsigned long initId = pMap->GetInitKFid();
  if ((kfs[0]->mnId == initId) == (kfs[1]->mnId == initId)) return refuse("exactly one keyframe must be the initial one");
  KF* k1 = kfs[0]->mnId == initId ? kfs[0] : kfs[1];
  KF* k2 = kfs[0]->mnId == initId ? kfs[1] : kfs[0];
  if (k1->mpCamera2 || k2->mpCamera2) return refuse("a keyframe has a second camera");
  {
    const auto T1 = k1->GetPose();
    const auto R1 = T1.rotationMatrix();
    const auto t1 = T1.translation();
    for (int r = 0; r < 3; ++r) {
      if (t1(r) != 0.f) return refuse("the fixed keyframe is not at the origin");
      for (int c = 0; c < 3; ++c) if (R1(r, c) != (r == c ? 1.f : 0.f)) return refuse("the fixed keyframe is rotated");
    }
  }
  InitialMapView v;
  const int n1 = (int)k1->mvKeysUn.size(), n2 = (int)k2->mvKeysUn.size();
  std::vector<morb_keypoint> keys1(n1), keys2(n2);
  auto conv = [](const auto& kp, morb_keypoint& o) { o.x = kp.pt.x; o.y = kp.pt.y; o.size = kp.size; o.angle = kp.angle; o.response = kp.response; o.octave = kp.octave; o.class_id = kp.class_id; };
  for (int i = 0; i < n1; ++i) conv(k1->mvKeysUn[i], keys1[i]);
  for (int i = 0; i < n2; ++i) conv(k2->mvKeysUn[i], keys2[i]);
  std::vector<int> m12(n1, -1);
  std::vector<uint8_t> tri(n1, 0);
  std::vector<float> p3d((size_t)n1 * 3, 0.f);
  std::vector<MP*> owner(n1, nullptr);
  for (MP* pMP : vpMP) {
    if (pMP->isBad()) continue;
    const auto obs = pMP->GetObservations();
    int i1 = -1, i2 = -1, others = 0;
    for (const auto& ob : obs) {
      const int left = std::get<0>(ob.second);
      if (ob.first == k1) i1 = left; else if (ob.first == k2) i2 = left; else if (!ob.first->isBad()) ++others;
    }
    if (others || i1 < 0 || i2 < 0 || i1 >= n1 || i2 >= n2) return refuse("a point is not observed by exactly the two keyframes");
    if (!(k1->mvuRight[i1] < 0) || !(k2->mvuRight[i2] < 0)) return refuse("a point has a stereo observation");
    if (owner[i1]) return refuse("two points share a keypoint");
    owner[i1] = pMP; m12[i1] = i2; tri[i1] = 1;
    const auto X = pMP->GetWorldPos();
    for (int k = 0; k < 3; ++k) p3d[3 * (size_t)i1 + k] = X(k);
  }
  v.n1 = n1; v.n2 = n2; v.keysUn1 = keys1.data(); v.keysUn2 = keys2.data(); v.matches12 = m12.data(); v.triangulated = tri.data(); v.P3D = p3d.data();
  {
    const auto T2 = k2->GetPose();
    const auto R2 = T2.rotationMatrix();
    const auto t2 = T2.translation();
    for (int r = 0; r < 3; ++r) { v.T21[9 + r] = t2(r); for (int c = 0; c < 3; ++c) v.T21[3 * r + c] = R2(r, c); }
  }
  v.nlevels = k2->mnScaleLevels;
  for (int l = 0; l < 16 && l < (int)k2->mvScaleFactors.size(); ++l) { v.scaleFactors[l] = k2->mvScaleFactors[l]; v.levelSigma2[l] = k2->mvLevelSigma2[l]; }
  const int np = (int)k2->mpCamera->size();
  v.kb8 = np == 8;
  for (int k = 0; k < np && k < 8; ++k) v.cam8[k] = k2->mpCamera->getParameter(k);
  v.depthScale = 0.f; v.minTracked = 0;
  BundleAdjustment(v, nIterations, bRobust, 0, pbStopFlag);
  using SE3 = typename std::decay<decltype(k2->GetPose())>::type;
  double R[9], t[3];
  for (int k = 0; k < 9; ++k) R[k] = v.Tcw2[k];
  for (int k = 0; k < 3; ++k) t[k] = v.Tcw2[9 + k];
  const bool own = nLoopKF == pMap->GetOriginKF()->mnId;
  if (own) k2->SetPose(se3_from_matrix<SE3>(R, t));                                    // :285-287 (the fixed keyframe keeps the pose it has)
  else {
    k1->mTcwGBA = k1->GetPose(); k1->mnBAGlobalForKF = nLoopKF;                         // :289-291
    k2->mTcwGBA = se3_from_matrix<SE3>(R, t); k2->mnBAGlobalForKF = nLoopKF;
  }
  for (int i = 0; i < n1; ++i) {                                                        // :345-361
    MP* pMP = owner[i];
    if (!pMP) continue;
    typename std::decay<decltype(pMP->GetWorldPos())>::type X;
    for (int k = 0; k < 3; ++k) X(k) = v.mpPos[3 * (size_t)i + k];
    if (own) { pMP->SetWorldPos(X); pMP->UpdateNormalAndDepth(); }
    else { pMP->mPosGBA = X; pMP->mnBAGlobalForKF = nLoopKF; }
  }
  return true;
}
template <class KF, class MP>
void Optimizer::BundleAdjustment(const std::vector<KF*>& vpKFs, const std::vector<MP*>& vpMP, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF,
                                 const bool bRobust) {
  std::string whyNot;
  if (initial_map_bundle_adjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust, &whyNot)) return;
#ifdef MORB_WHOLE_MAP_BUNDLE_ADJUSTMENT
  WholeMapBundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust);
#else
  throw std::runtime_error(whyNot);
#endif
}

// The graph Optimizer::BundleAdjustment assembles at Optimizer.cc:113-268, flattened on the host (no device call: tests/native/
// global_ba_member_check.cc checks it alone).  Vertices: the keyframes of vpKFs that are not bad, by ascending mnId (the order the solver's
// envelope wants; g2o orders by id itself), the one with GetInitKFid() fixed (:121); the points of vpMP that are not bad and carry an edge
// (:262-267), in vpMP's order.  Edges in the reference's order — by point, within a point by GetObservations()'s iteration, the left
// observation (monocular: mvuRight < 0, else stereo, :155-221) before the right camera's (:223-259) — skipping an observation by a bad
// keyframe, by one with mnId > maxKFid or by one that is not in vpKFs (:148-150).
template <class KF, class MP>
struct WholeMapFlat {
  std::vector<KF*> kfs;
  std::vector<MP*> mps;
  std::vector<float> kfPose, mpPos, eObs, eInv;
  std::vector<uint8_t> kfFixed, eRight;
  std::vector<int> eKF, eMP;
  bool rig = false;   // a keyframe has a second camera: every left observation is an EdgeSE3ProjectXYZ on the KannalaBrandt8 camera
};
namespace morb_glue {
template <class KF, class MP>
void flatten_whole_map(const std::vector<KF*>& vpKFs, const std::vector<MP*>& vpMP, WholeMapFlat<KF, MP>& f) {
  for (KF* k : vpKFs) if (!k->isBad()) f.kfs.push_back(k);
  std::stable_sort(f.kfs.begin(), f.kfs.end(), [](KF* a, KF* b) { return a->mnId < b->mnId; });
  if (f.kfs.empty()) return;
  const unsigned long initId = vpKFs[0]->GetMap()->GetInitKFid();
  std::map<KF*, int> kfIndex;
  unsigned long maxKFid = 0;
  for (KF* k : f.kfs) {
    const int at = (int)kfIndex.size();
    kfIndex[k] = at;
    float p[7];
    pose7(k->GetPose(), p);
    f.kfPose.insert(f.kfPose.end(), p, p + 7);
    f.kfFixed.push_back(k->mnId == initId ? 1 : 0);
    if (k->mnId > maxKFid) maxKFid = k->mnId;
    if (k->mpCamera2) f.rig = true;
  }
  for (MP* pMP : vpMP) {
    if (pMP->isBad()) continue;
    const int j = (int)f.mps.size();
    const size_t before = f.eKF.size();
    for (const auto& ob : pMP->GetObservations()) {
      KF* pKF = ob.first;
      if (pKF->isBad() || pKF->mnId > maxKFid) continue;
      const auto it = kfIndex.find(pKF);
      if (it == kfIndex.end()) continue;   // (optimizer.vertex(pKF->mnId) == NULL)
      const int leftIndex = std::get<0>(ob.second);
      if (leftIndex != -1) {
        const auto& kpUn = pKF->mvKeysUn[leftIndex];
        const float ur = pKF->mvuRight[leftIndex];
        if (f.rig && !(ur < 0)) throw std::runtime_error("Optimizer::BundleAdjustment: a stereo observation in a map of KannalaBrandt8 rigs");
        f.eKF.push_back(it->second); f.eMP.push_back(j); f.eRight.push_back(0);
        f.eObs.push_back(kpUn.pt.x); f.eObs.push_back(kpUn.pt.y); f.eObs.push_back(ur < 0 ? -1.f : ur);
        f.eInv.push_back(pKF->mvInvLevelSigma2[kpUn.octave]);
      }
      if (pKF->mpCamera2) {
        int rightIndex = std::get<1>(ob.second);
        if (rightIndex != -1 && rightIndex < static_cast<int>(pKF->mvKeysRight.size())) {   // (:226, as the reference tests it)
          rightIndex -= pKF->NLeft;
          const auto& kp = pKF->mvKeysRight[rightIndex];
          f.eKF.push_back(it->second); f.eMP.push_back(j); f.eRight.push_back(1);
          f.eObs.push_back(kp.pt.x); f.eObs.push_back(kp.pt.y); f.eObs.push_back(-1.f);
          f.eInv.push_back(pKF->mvInvLevelSigma2[kp.octave]);
        }
      }
    }
    if (f.eKF.size() == before) continue;   // :262-264: the vertex is removed again
    f.mps.push_back(pMP);
    const auto X = pMP->GetWorldPos();
    f.mpPos.push_back(X(0)); f.mpPos.push_back(X(1)); f.mpPos.push_back(X(2));
  }
}
}  // namespace morb_glue

// Optimizer::BundleAdjustment (Optimizer.cc:56-362) over any map: flattened as above, solved by the view form (morb_bundle_adjustment*), written
// back as :276-361 does — SetPose / SetWorldPos / UpdateNormalAndDepth when nLoopKF is the origin keyframe's id, else mTcwGBA / mPosGBA /
// mnBAGlobalForKF; every keyframe that is not bad is written (a fixed one, or one without an edge, with the pose it has), as the reference
// does.  A raised *pbStopFlag stops the optimisation, not the write-back.  The `dist > 1` block of :297-340 only counts and is left out.
template <class KF, class MP>
void Optimizer::WholeMapBundleAdjustment(const std::vector<KF*>& vpKFs, const std::vector<MP*>& vpMP, int nIterations, bool* pbStopFlag,
                                         const unsigned long nLoopKF, const bool bRobust) {
  using SE3 = typename std::decay<decltype(vpKFs[0]->GetPose())>::type;
  WholeMapFlat<KF, MP> f;
  morb_glue::flatten_whole_map(vpKFs, vpMP, f);
  if (f.kfs.empty()) return;
  auto* pMap = vpKFs[0]->GetMap();
  if (!f.eKF.empty()) {
    GlobalBAView g;
    g.nKF = (int)f.kfs.size(); g.nMP = (int)f.mps.size(); g.nE = (int)f.eKF.size();
    g.kfPose = f.kfPose.data(); g.kfFixed = f.kfFixed.data(); g.mpPos = f.mpPos.data(); g.eKF = f.eKF.data(); g.eMP = f.eMP.data();
    g.eObs = f.eObs.data(); g.eInvSigma2 = f.eInv.data();
    KF* k0 = f.kfs[0];
    g.fx = k0->fx; g.fy = k0->fy; g.cx = k0->cx; g.cy = k0->cy; g.mbf = k0->mbf;
    float rigp[28];
    if (f.rig) {
      KF* kr = nullptr;
      for (KF* k : f.kfs) if (k->mpCamera2) { kr = k; break; }
      morb_glue::rig28(kr, rigp); g.rig28 = rigp; g.eRight = f.eRight.data();
    }
    BundleAdjustment(g, nIterations, bRobust, pbStopFlag);
  }
  const bool own = nLoopKF == pMap->GetOriginKF()->mnId;
  for (size_t i = 0; i < f.kfs.size(); ++i) {   // :278-342
    KF* pKF = f.kfs[i];
    const SE3 T = morb_glue::make_se3<SE3>(&f.kfPose[7 * i]);
    if (own) pKF->SetPose(T);
    else { pKF->mTcwGBA = T; pKF->mnBAGlobalForKF = nLoopKF; }
  }
  for (size_t j = 0; j < f.mps.size(); ++j) {   // :345-361
    MP* pMP = f.mps[j];
    typename std::decay<decltype(pMP->GetWorldPos())>::type X;
    for (int k = 0; k < 3; ++k) X(k) = f.mpPos[3 * j + k];
    if (own) { pMP->SetWorldPos(X); pMP->UpdateNormalAndDepth(); }
    else { pMP->mPosGBA = X; pMP->mnBAGlobalForKF = nLoopKF; }
  }
}

// void Optimizer::LocalBundleAdjustment(KeyFrame* pMainKF, vector<KeyFrame*> vpAdjustKF, vector<KeyFrame*> vpFixedKF, bool* pbStopFlag)
// Optimizer.cc:3430-3851, the welding bundle adjustment of LoopClosing::MergeLocal (call site LoopClosing.cc:1652-1653).  The graph selection
// with its marks (mnBALocalForMerge), flattened; the erase list, the poses and the points written back under mMutexMapUpdate.  The per-keyframe
// counters and the mpObs* maps of the reference only count and are not kept.  One deviation: on a KannalaBrandt8 rig an observation by the
// right camera alone (left index -1) is skipped — the reference indexes mvpMapPoints[-1] there.
template <class KF>
void Optimizer::LocalBundleAdjustment(KF* pMainKF, std::vector<KF*> vpAdjustKF, std::vector<KF*> vpFixedKF, bool* pbStopFlag) {
  using SE3 = typename std::decay<decltype(pMainKF->GetPose())>::type;
  using MP = typename std::remove_pointer<typename std::decay<decltype(*pMainKF->GetMapPoints().begin())>::type>::type;
  auto* pCurrentMap = pMainKF->GetMap();
  const auto mainId = pMainKF->mnId;
  std::vector<MP*> vpMPs;
  std::map<KF*, int> kfIndex;
  std::vector<KF*> kfs;
  std::vector<float> kfPose;
  std::vector<uint8_t> kfFixed;
  long unsigned int maxKFid = 0;
  auto add_window = [&](const std::vector<KF*>& window, bool fixed) {   // :3459-3492 (fixed), :3494-3524 (free)
    for (KF* pKFi : window) {
      if (pKFi->isBad() || pKFi->GetMap() != pCurrentMap) continue;
      pKFi->mnBALocalForMerge = mainId;
      if (!kfIndex.count(pKFi)) {   // (a keyframe of both windows keeps its first vertex: g2o refuses the second id)
        kfIndex[pKFi] = (int)kfs.size(); kfs.push_back(pKFi);
        float p[7];
        morb_glue::pose7(pKFi->GetPose(), p);
        kfPose.insert(kfPose.end(), p, p + 7);
        kfFixed.push_back(fixed ? 1 : 0);
      }
      if (pKFi->mnId > maxKFid) maxKFid = pKFi->mnId;
      for (MP* pMPi : pKFi->GetMapPoints())
        if (pMPi && !pMPi->isBad() && pMPi->GetMap() == pCurrentMap && pMPi->mnBALocalForMerge != mainId) {
          vpMPs.push_back(pMPi);
          pMPi->mnBALocalForMerge = mainId;
        }
    }
  };
  add_window(vpFixedKF, true);
  add_window(vpAdjustKF, false);
  // :3550-3648 — points and edges
  const bool kb8 = pMainKF->mpCamera && pMainKF->mpCamera->size() == 8;
  std::vector<MP*> mps;
  std::vector<float> mpPos, eObs, eInv;
  std::vector<int> eKF, eMP;
  std::vector<std::pair<KF*, MP*>> eOwner;
  for (MP* pMPi : vpMPs) {
    if (pMPi->isBad()) continue;
    const int j = (int)mps.size();
    mps.push_back(pMPi);
    const auto X = pMPi->GetWorldPos();
    mpPos.push_back(X(0)); mpPos.push_back(X(1)); mpPos.push_back(X(2));
    for (const auto& ob : pMPi->GetObservations()) {
      KF* pKF = ob.first;
      const int leftIndex = std::get<0>(ob.second);
      if (leftIndex < 0) continue;   // (the deviation named above)
      if (pKF->isBad() || pKF->mnId > maxKFid || pKF->mnBALocalForMerge != mainId || !pKF->GetMapPoint(leftIndex)) continue;
      const auto it = kfIndex.find(pKF);
      if (it == kfIndex.end()) continue;   // (marked by an earlier call with this main keyframe, no vertex now: optimizer.vertex(id) would be NULL)
      const auto& kpUn = pKF->mvKeysUn[leftIndex];
      eKF.push_back(it->second); eMP.push_back(j);
      eObs.push_back(kpUn.pt.x); eObs.push_back(kpUn.pt.y); eObs.push_back(pKF->mvuRight[leftIndex] < 0 ? -1.f : pKF->mvuRight[leftIndex]);
      eInv.push_back(pKF->mvInvLevelSigma2[kpUn.octave]);
      eOwner.emplace_back(pKF, pMPi);
    }
  }
  if (pbStopFlag && *pbStopFlag) return;   // :3650-3651
  MergeBAView g;
  g.nKF = (int)kfs.size(); g.nMP = (int)mps.size(); g.nE = (int)eKF.size();
  if (g.nKF == 0 || g.nMP == 0 || g.nE == 0) return;   // (an empty graph: g2o optimises nothing and every write-back is the identity)
  g.kfPose = kfPose.data(); g.kfFixed = kfFixed.data(); g.mpPos = mpPos.data(); g.eKF = eKF.data(); g.eMP = eMP.data();
  g.eObs = eObs.data(); g.eInvSigma2 = eInv.data();
  g.fx = pMainKF->fx; g.fy = pMainKF->fy; g.cx = pMainKF->cx; g.cy = pMainKF->cy; g.mbf = pMainKF->mbf;
  float camL[8];
  if (kb8) { morb_glue::cam8(pMainKF->mpCamera, camL); g.camL8 = camL; }
  LocalBundleAdjustment(g, pbStopFlag);
  if (g.stats[5] == 0) return;             // (the flag was raised between the check above and the entry's own)
  std::unique_lock<std::mutex> lock(pMainKF->GetMap()->mMutexMapUpdate);   // :3747
  for (size_t e = 0; e < eOwner.size(); ++e)                               // :3749-3756
    if (g.eraseFlag[e] && !eOwner[e].second->isBad()) {
      eOwner[e].first->EraseMapPointMatch(eOwner[e].second);
      eOwner[e].second->EraseObservation(eOwner[e].first);
    }
  for (KF* pKFi : vpAdjustKF) {                                            // :3784-3840
    if (pKFi->isBad()) continue;
    const auto it = kfIndex.find(pKFi);
    if (it == kfIndex.end() || kfFixed[it->second]) continue;
    pKFi->SetPose(morb_glue::make_se3<SE3>(&kfPose[(size_t)7 * it->second]));
  }
  for (int j = 0; j < (int)mps.size(); ++j) {                              // :3843-3850
    if (mps[j]->isBad()) continue;
    typename std::decay<decltype(mps[j]->GetWorldPos())>::type X;
    for (int k = 0; k < 3; ++k) X(k) = mpPos[3 * j + k];
    mps[j]->SetWorldPos(X);
    mps[j]->UpdateNormalAndDepth();
  }
}

// void Optimizer::MergeInertialBA(KeyFrame* pCurrKF, KeyFrame* pMergeKF, bool* pbStopFlag, Map* pMap, LoopClosing::KeyFrameAndPose& corrPoses)
// Optimizer.cc:3853-4389, the welding bundle adjustment of an inertial map merge (call sites LoopClosing.cc:1649-1650, :2099).  The window
// and covisible selection with its marks (:3856-3983), flattened: the 15-unknown keyframes are vpOptimizableKFs and vpOptimizableCovKFs[0]
// when a link hangs on it (kind 0), the further covisible keyframes and every keyframe with !bImu are free in the pose only (kind 3), the
// one keyframe of lFixedKeyFrames is kind 1 (kind 2 without an IMU state).  The erase list, poses, velocities, biases, corrPoses and the
// points are written back under mMutexMapUpdate.  CorrMap = LoopClosing::KeyFrameAndPose (a map from KeyFrame* to g2o::Sim3).
template <class KF, class MapT, class CorrMap>
void Optimizer::MergeInertialBA(KF* pCurrKF, KF* pMergeKF, bool* pbStopFlag, MapT* pMap, CorrMap& corrPoses) {
  using SE3 = typename std::decay<decltype(pCurrKF->GetPose())>::type;
  using MP = typename std::remove_pointer<typename std::decay<decltype(pCurrKF->GetMapPointMatches()[0])>::type>::type;
  using Bias = typename std::decay<decltype(pCurrKF->GetImuBias())>::type;
  using Sim3T = typename CorrMap::mapped_type;
  const int Nd = 6;                                                                     // :3856
  const unsigned long maxKFid = pCurrKF->mnId;
  const auto id = pCurrKF->mnId;
  std::vector<KF*> vpOptimizableKFs, vpOptimizableCovKFs;
  vpOptimizableKFs.reserve(2 * Nd);
  const int maxCovKF = 30;                                                              // :3864
  vpOptimizableCovKFs.reserve(maxCovKF);
  vpOptimizableKFs.push_back(pCurrKF);                                                  // :3869-3877: the current keyframe's window
  pCurrKF->mnBALocalForKF = id;
  for (int i = 1; i < Nd; i++) {
    if (vpOptimizableKFs.back()->mPrevKF) {
      vpOptimizableKFs.push_back(vpOptimizableKFs.back()->mPrevKF);
      vpOptimizableKFs.back()->mnBALocalForKF = id;
    } else break;
  }
  std::list<KF*> lFixedKeyFrames;                                                       // :3879-3886: the head of the current chain
  if (vpOptimizableKFs.back()->mPrevKF) {
    vpOptimizableCovKFs.push_back(vpOptimizableKFs.back()->mPrevKF);
    vpOptimizableKFs.back()->mPrevKF->mnBALocalForKF = id;
  } else {
    vpOptimizableCovKFs.push_back(vpOptimizableKFs.back());
    vpOptimizableKFs.pop_back();
  }
  vpOptimizableKFs.push_back(pMergeKF);                                                 // :3889-3899: the merge keyframe and its predecessors
  pMergeKF->mnBALocalForKF = id;
  for (int i = 1; i < (Nd / 2); i++) {
    if (vpOptimizableKFs.back()->mPrevKF) {
      vpOptimizableKFs.push_back(vpOptimizableKFs.back()->mPrevKF);
      vpOptimizableKFs.back()->mnBALocalForKF = id;
    } else break;
  }
  if (vpOptimizableKFs.back()->mPrevKF) {                                               // :3902-3910: "we fix just once the old map"
    lFixedKeyFrames.push_back(vpOptimizableKFs.back()->mPrevKF);
    vpOptimizableKFs.back()->mPrevKF->mnBAFixedForKF = id;
  } else {
    vpOptimizableKFs.back()->mnBALocalForKF = 0;
    vpOptimizableKFs.back()->mnBAFixedForKF = id;
    lFixedKeyFrames.push_back(vpOptimizableKFs.back());
    vpOptimizableKFs.pop_back();
  }
  if (pMergeKF->mNextKF) {                                                              // :3913-3924: its successors
    vpOptimizableKFs.push_back(pMergeKF->mNextKF);
    vpOptimizableKFs.back()->mnBALocalForKF = id;
  }
  while (vpOptimizableKFs.size() < (size_t)(2 * Nd)) {
    if (vpOptimizableKFs.back()->mNextKF) {
      vpOptimizableKFs.push_back(vpOptimizableKFs.back()->mNextKF);
      vpOptimizableKFs.back()->mnBALocalForKF = id;
    } else break;
  }
  int N = (int)vpOptimizableKFs.size();
  std::list<MP*> lLocalMapPoints;                                                       // :3929-3950
  std::map<MP*, int> mLocalObs;
  for (int i = 0; i < N; i++)
    for (MP* pMP : vpOptimizableKFs[i]->GetMapPointMatches())
      if (pMP && !pMP->isBad()) {
        if (pMP->mnBALocalForKF != id) { mLocalObs[pMP] = 1; lLocalMapPoints.push_back(pMP); pMP->mnBALocalForKF = id; }
        else mLocalObs[pMP]++;
      }
  std::vector<std::pair<MP*, int>> pairs;                                               // :3952-3956
  pairs.reserve(mLocalObs.size());
  for (auto itr = mLocalObs.begin(); itr != mLocalObs.end(); ++itr) pairs.push_back(*itr);
  std::sort(pairs.begin(), pairs.end(), [](const std::pair<MP*, int>& a, const std::pair<MP*, int>& b) { return a.second < b.second; });   // sortByVal (:43-45)
  {                                                                                     // :3960-3983: one covisible keyframe per point, at most maxCovKF points
    int i = 0;
    for (auto lit = pairs.begin(), lend = pairs.end(); lit != lend; lit++, i++) {
      auto observations = lit->first->GetObservations();
      if (i >= maxCovKF) break;
      for (auto mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
        KF* pKFi = mit->first;
        if (pKFi->mnBALocalForKF != id && pKFi->mnBAFixedForKF != id) {
          pKFi->mnBALocalForKF = id;
          if (!pKFi->isBad()) { vpOptimizableCovKFs.push_back(pKFi); break; }
        }
      }
    }
  }
  // inertial links (:4082-4150), found before the vertices so that a keyframe's width is known: a link needs bImu on both ends, the
  // preintegration, and a vertex for its predecessor
  std::map<KF*, int> kfIndex;
  std::vector<KF*> kfs;
  auto listed = [&](KF* k) {
    if (std::find(vpOptimizableKFs.begin(), vpOptimizableKFs.end(), k) != vpOptimizableKFs.end()) return true;
    if (std::find(vpOptimizableCovKFs.begin(), vpOptimizableCovKFs.end(), k) != vpOptimizableCovKFs.end()) return true;
    return std::find(lFixedKeyFrames.begin(), lFixedKeyFrames.end(), k) != lFixedKeyFrames.end();
  };
  std::vector<std::pair<KF*, KF*>> links;
  for (int i = 0; i < N; i++) {
    KF* pKFi = vpOptimizableKFs[i];
    if (!pKFi->mPrevKF) continue;
    if (!(pKFi->bImu && pKFi->mPrevKF->bImu && pKFi->mpImuPreintegrated)) continue;
    pKFi->mpImuPreintegrated->SetNewBias(pKFi->mPrevKF->GetImuBias());                  // :4092
    if (!listed(pKFi->mPrevKF)) continue;                                               // (:4108-4113: a vertex is missing)
    links.emplace_back(pKFi->mPrevKF, pKFi);
  }
  auto linked = [&](KF* k) { for (const auto& l : links) if (l.first == k || l.second == k) return true; return false; };
  // vertices (:4001-4076)
  std::vector<float> kfState;
  std::vector<uint8_t> kfKind;
  auto add_kf = [&](KF* k, int kind) {
    if (kfIndex.count(k)) return;   // (g2o refuses a second vertex with the same id)
    kfIndex[k] = (int)kfs.size(); kfs.push_back(k);
    float s[21];
    morb_glue::imu_state21(k, s); morb_glue::bias6(k->GetImuBias(), s + 15);
    kfState.insert(kfState.end(), s, s + 21);
    kfKind.push_back((uint8_t)kind);
  };
  for (KF* k : vpOptimizableKFs) add_kf(k, k->bImu ? 0 : 3);
  for (KF* k : vpOptimizableCovKFs) add_kf(k, k->bImu && linked(k) ? 0 : 3);   // (velocity and biases of the others carry no edge)
  for (KF* k : lFixedKeyFrames) add_kf(k, k->bImu ? 1 : 2);
  std::vector<int> iKF1, iKF2;
  std::vector<morb_imu_preintegrated> iPre;
  for (const auto& l : links) {
    iKF1.push_back(kfIndex[l.first]); iKF2.push_back(kfIndex[l.second]);
    iPre.emplace_back(); morb_glue::fill_pre(iPre.back(), l.second->mpImuPreintegrated);
  }
  // points and visual edges (:4185-4272)
  std::vector<MP*> mps(lLocalMapPoints.begin(), lLocalMapPoints.end());
  std::vector<float> mpPos, eObs, eInv;
  std::vector<int> eKF, eMP;
  std::vector<std::pair<KF*, MP*>> eOwner;
  for (int j = 0; j < (int)mps.size(); ++j) {
    MP* pMP = mps[j];
    const auto X = pMP->GetWorldPos();
    mpPos.push_back(X(0)); mpPos.push_back(X(1)); mpPos.push_back(X(2));
    for (const auto& ob : pMP->GetObservations()) {
      KF* pKFi = ob.first;
      if (!pKFi) continue;
      if (pKFi->mnBALocalForKF != id && pKFi->mnBAFixedForKF != id) continue;
      if (pKFi->mnId > maxKFid) continue;                                               // :4214
      const auto it = kfIndex.find(pKFi);
      if (it == kfIndex.end() || pKFi->isBad()) continue;                               // :4218-4221
      const int leftIndex = std::get<0>(ob.second);
      if (leftIndex < 0) continue;   // (a right-camera-only observation: the reference indexes mvKeysUn[-1] there)
      const auto& kpUn = pKFi->mvKeysUn[leftIndex];
      eKF.push_back(it->second); eMP.push_back(j);
      eObs.push_back(kpUn.pt.x); eObs.push_back(kpUn.pt.y); eObs.push_back(pKFi->mvuRight[leftIndex] < 0 ? -1.f : pKFi->mvuRight[leftIndex]);
      eInv.push_back(pKFi->mvInvLevelSigma2[kpUn.octave]);
      eOwner.emplace_back(pKFi, pMP);
    }
  }
  if (pbStopFlag && *pbStopFlag) return;                                                // :4276-4277
  MergeInertialBAView g;
  g.nKF = (int)kfs.size(); g.nMP = (int)mps.size(); g.nE = (int)eKF.size(); g.nI = (int)iKF1.size();
  auto corr_of = [&](KF* pKFi) {   // corrPoses[pKFi] = g2o::Sim3(Tiw.unit_quaternion(), Tiw.translation(), 1.0) of the keyframe's float pose
    using Quat = typename std::decay<decltype(std::declval<Sim3T>().rotation())>::type;
    using Vec3 = typename std::decay<decltype(std::declval<Sim3T>().translation())>::type;
    const auto Tiw = pKFi->GetPose();
    const auto q = Tiw.unit_quaternion();
    const auto t = Tiw.translation();
    Vec3 tv;
    for (int k = 0; k < 3; ++k) tv(k) = (double)t(k);
    corrPoses[pKFi] = Sim3T(Quat((double)q.w(), (double)q.x(), (double)q.y(), (double)q.z()), tv, 1.0);
  };
  if (g.nMP == 0 || g.nE == 0) {   // no point, no edge: nothing for the device.  g2o optimises nothing there and the reference writes every estimate
    // back as it stands — what a caller sees of that is corrPoses of every keyframe of the windows and the map's change index
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    for (KF* k : vpOptimizableKFs) corr_of(k);
    for (KF* k : vpOptimizableCovKFs) corr_of(k);
    pMap->IncreaseChangeIndex();
    return;
  }
  g.kfState = kfState.data(); g.kfKind = kfKind.data(); g.mpPos = mpPos.data(); g.eKF = eKF.data(); g.eMP = eMP.data();
  g.eObs = eObs.data(); g.eInvSigma2 = eInv.data();
  const int noLink = 0; const morb_imu_preintegrated noPre{};
  g.iKF1 = g.nI ? iKF1.data() : &noLink; g.iKF2 = g.nI ? iKF2.data() : &noLink; g.iPre = g.nI ? iPre.data() : &noPre;
  g.fx = pCurrKF->fx; g.fy = pCurrKF->fy; g.cx = pCurrKF->cx; g.cy = pCurrKF->cy; g.mbf = pCurrKF->mbf;
  morb_glue::tbc12(pCurrKF->mImuCalib.mTbc, g.Tbc12);
  float rigp[28];
  if (pCurrKF->mpCamera2) { morb_glue::rig28(pCurrKF, rigp); g.rig28 = rigp; }
  MergeInertialBA(g, pbStopFlag);
  if (!g.ran) return;                      // (the flag was raised between the check above and the entry's own)
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                             // :4313
  for (size_t e = 0; e < eOwner.size(); ++e)                                            // :4287-4321
    if (g.eraseFlag[e] && !eOwner[e].second->isBad()) {
      eOwner[e].first->EraseMapPointMatch(eOwner[e].second);
      eOwner[e].second->EraseObservation(eOwner[e].first);
    }
  // :4325-4375: Tcw = (Rcb Rwb^T, tcb - Rcb Rwb^T twb) (ImuCamPose, G2oTypes.cc:74-113), corrPoses, velocity, bias
  float Tbc[12];
  morb_glue::tbc12(pCurrKF->mImuCalib.mTbc, Tbc);
  auto write_back = [&](KF* pKFi) {
    const int row = kfIndex[pKFi];
    const float* s = &kfState[(size_t)21 * row];
    double Rcw[9], tcw[3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) { double a = 0; for (int k = 0; k < 3; ++k) a += (double)Tbc[3 * k + r] * s[3 * c + k]; Rcw[3 * r + c] = a; }   // Rcb Rwb^T, Rcb = Rbc^T
    for (int r = 0; r < 3; ++r) {
      double a = 0;
      for (int k = 0; k < 3; ++k) a -= (double)Tbc[3 * k + r] * Tbc[9 + k];            // tcb = -Rbc^T tbc
      for (int c = 0; c < 3; ++c) a -= Rcw[3 * r + c] * s[9 + c];
      tcw[r] = a;
    }
    pKFi->SetPose(se3_from_matrix<SE3>(Rcw, tcw));
    corr_of(pKFi);   // (of the float pose just set)
    if (pKFi->bImu && kfKind[row] == 0) {
      typename std::decay<decltype(pKFi->GetVelocity())>::type vel;
      for (int k = 0; k < 3; ++k) vel(k) = s[12 + k];
      pKFi->SetVelocity(vel);
      pKFi->SetNewBias(Bias(s[18], s[19], s[20], s[15], s[16], s[17]));
    }
    // (kind 3 with bImu: the reference writes the vertices' estimates back, which never left the keyframe's own velocity and bias)
  };
  for (KF* k : vpOptimizableKFs) write_back(k);
  for (KF* k : vpOptimizableCovKFs) write_back(k);
  for (int j = 0; j < (int)mps.size(); ++j) {                                           // :4378-4386
    typename std::decay<decltype(mps[j]->GetWorldPos())>::type X;
    for (int k = 0; k < 3; ++k) X(k) = mpPos[3 * j + k];
    mps[j]->SetWorldPos(X);
    mps[j]->UpdateNormalAndDepth();
  }
  pMap->IncreaseChangeIndex();                                                          // :4388
}

// void Optimizer::FullInertialBA(Map* pMap, int its, const bool bFixLocal, const unsigned long nLoopId, bool* pbStopFlag, bool bInit, float priorG,
// float priorA, Eigen::VectorXd* vSingVal, bool* bHess)  Optimizer.cc:364-760, the inertial whole-map bundle adjustment (call sites
// LoopClosing.cc:2305 and LocalMapping.cc:1244-1249).  The map flattened as morb_full_inertial_ba takes it: a vertex per keyframe with mnId <=
// maxKFid, by ascending mnId; what bFixLocal fixes (:401-406) with the return below three free keyframes (:438-440); a link per keyframe with
// mPrevKF, both bImu, neither bad nor beyond maxKFid, whose predecessor has a vertex, after SetNewBias(mPrevKF->GetImuBias()) (:443-533); kind 0 /
// 1 for a bImu keyframe that enters a link, 3 / 2 otherwise (velocity and bias vertices without an edge are not in g2o's active set); the
// observations of every point by the keyframes that are not bad, the left before the right one, a point seen by fixed keyframes alone without
// edges and not written (:683-686, :744); with bInit the last keyframe's bias (pIncKF) as the shared one.  Written back as :696-759 does: SetPose /
// SetVelocity / SetNewBias / SetWorldPos / UpdateNormalAndDepth when nLoopId == 0, else mTcwGBA / mVwbGBA / mBiasGBA / mPosGBA / mnBAGlobalForKF;
// with bInit every bImu keyframe gets the shared bias; then IncreaseChangeIndex().  The handle: LocalMapping's calls pass no stop flag
// (kMapping), LoopClosing's does (kLoopClosing) — nLoopId cannot tell them apart, LocalMapping passes a keyframe id there.  A map without a
// usable observation is written back as it stands.  vSingVal and bHess are not touched, as in the reference.
template <class MapT, class VecX>
void Optimizer::FullInertialBA(MapT* pMap, int its, const bool bFixLocal, const unsigned long nLoopId, bool* pbStopFlag, bool bInit, float priorG,
                               float priorA, VecX*, bool*) {
  const unsigned long maxKFid = pMap->GetMaxKFid();
  const auto vpKFs = pMap->GetAllKeyFrames();
  const auto vpMPs = pMap->GetAllMapPoints();
  using KF = typename std::remove_pointer<typename std::decay<decltype(vpKFs[0])>::type>::type;
  using MP = typename std::remove_pointer<typename std::decay<decltype(vpMPs[0])>::type>::type;
  using SE3 = typename std::decay<decltype(vpKFs[0]->GetPose())>::type;
  using Bias = typename std::decay<decltype(vpKFs[0]->GetImuBias())>::type;
  // vertices (:392-436)
  std::vector<KF*> kfs;
  KF* pIncKF = nullptr;
  for (KF* k : vpKFs) {
    if (k->mnId > maxKFid) continue;
    kfs.push_back(k);
    pIncKF = k;
  }
  if (kfs.empty()) return;
  std::stable_sort(kfs.begin(), kfs.end(), [](KF* a, KF* b) { return a->mnId < b->mnId; });
  std::map<KF*, int> kfIndex;
  std::vector<uint8_t> fixed(kfs.size(), 0);
  int nNonFixed = 0;
  for (size_t i = 0; i < kfs.size(); ++i) {
    kfIndex[kfs[i]] = (int)i;
    if (bFixLocal) {
      fixed[i] = (kfs[i]->mnBALocalForKF >= (maxKFid - 1)) || (kfs[i]->mnBAFixedForKF >= (maxKFid - 1)) ? 1 : 0;
      if (!fixed[i]) nNonFixed++;
    }
  }
  if (bFixLocal && nNonFixed < 3) return;                                               // :438-440
  // links (:443-533), in the order of GetAllKeyFrames()
  std::vector<int> iKF1, iKF2;
  std::vector<morb_imu_preintegrated> iPre;
  std::vector<uint8_t> linked(kfs.size(), 0);
  for (KF* pKFi : vpKFs) {
    if (!pKFi->mPrevKF || pKFi->mnId > maxKFid) continue;
    if (pKFi->isBad() || pKFi->mPrevKF->mnId > maxKFid) continue;
    if (!(pKFi->bImu && pKFi->mPrevKF->bImu)) continue;
    pKFi->mpImuPreintegrated->SetNewBias(pKFi->mPrevKF->GetImuBias());                  // :455
    const auto it1 = kfIndex.find(pKFi->mPrevKF);
    if (it1 == kfIndex.end()) continue;                                                 // (:479-491: a vertex is missing)
    const int r1 = it1->second, r2 = kfIndex[pKFi];
    iKF1.push_back(r1); iKF2.push_back(r2);
    iPre.emplace_back(); morb_glue::fill_pre(iPre.back(), pKFi->mpImuPreintegrated);
    linked[r1] = linked[r2] = 1;
  }
  std::vector<float> kfState;
  std::vector<uint8_t> kfKind;
  bool rig = false;
  for (size_t i = 0; i < kfs.size(); ++i) {
    float s[21];
    morb_glue::imu_state21(kfs[i], s); morb_glue::bias6(kfs[i]->GetImuBias(), s + 15);
    kfState.insert(kfState.end(), s, s + 21);
    const bool imu = kfs[i]->bImu && linked[i];
    kfKind.push_back((uint8_t)(fixed[i] ? (imu ? 1 : 2) : (imu ? 0 : 3)));
    if (kfs[i]->mpCamera2) rig = true;
  }
  // points and visual edges (:563-687)
  std::vector<float> mpPos, eObs, eInv;
  std::vector<int> eKF, eMP;
  std::vector<uint8_t> eRight, included(vpMPs.size(), 0);
  for (size_t j = 0; j < vpMPs.size(); ++j) {
    MP* pMP = vpMPs[j];
    const auto X = pMP->GetWorldPos();
    mpPos.push_back(X(0)); mpPos.push_back(X(1)); mpPos.push_back(X(2));
    const size_t before = eKF.size();
    bool bAllFixed = true;
    for (const auto& ob : pMP->GetObservations()) {
      KF* pKFi = ob.first;
      if (pKFi->mnId > maxKFid || pKFi->isBad()) continue;
      const auto it = kfIndex.find(pKFi);
      if (it == kfIndex.end()) continue;   // (optimizer.vertex(pKFi->mnId) == NULL: the reference dereferences it)
      const int leftIndex = std::get<0>(ob.second);
      if (leftIndex != -1) {
        const auto& kpUn = pKFi->mvKeysUn[leftIndex];
        const float ur = pKFi->mvuRight[leftIndex];
        eKF.push_back(it->second); eMP.push_back((int)j); eRight.push_back(0);
        eObs.push_back(kpUn.pt.x); eObs.push_back(kpUn.pt.y); eObs.push_back(ur < 0 ? -1.f : ur);
        eInv.push_back(pKFi->mvInvLevelSigma2[kpUn.octave]);
        if (!fixed[it->second]) bAllFixed = false;
      }
      if (pKFi->mpCamera2) {
        int rightIndex = std::get<1>(ob.second);
        if (rightIndex != -1 && rightIndex < static_cast<int>(pKFi->mvKeysRight.size())) {   // (:651, as the reference tests it)
          rightIndex -= pKFi->NLeft;
          const auto& kp = pKFi->mvKeysRight[rightIndex];
          eKF.push_back(it->second); eMP.push_back((int)j); eRight.push_back(1);
          eObs.push_back(kp.pt.x); eObs.push_back(kp.pt.y); eObs.push_back(-1.f);
          eInv.push_back(pKFi->mvInvLevelSigma2[kp.octave]);
          if (!fixed[it->second]) bAllFixed = false;
        }
      }
    }
    if (bAllFixed) { eKF.resize(before); eMP.resize(before); eRight.resize(before); eObs.resize(3 * before); eInv.resize(before); }   // :683-686
    else included[j] = 1;
  }
  if (pbStopFlag && *pbStopFlag) return;                                                // :689-690
  FullInertialBAView g;
  g.nKF = (int)kfs.size(); g.nMP = (int)vpMPs.size(); g.nE = (int)eKF.size(); g.nI = (int)iKF1.size();
  morb_glue::bias6(pIncKF->GetImuBias(), g.bias6);                                      // :428-435
  KF* k0 = kfs[0];
  morb_glue::tbc12(k0->mImuCalib.mTbc, g.Tbc12);
  if (g.nE > 0) {
    g.kfState = kfState.data(); g.kfKind = kfKind.data(); g.mpPos = mpPos.data(); g.eKF = eKF.data(); g.eMP = eMP.data();
    g.eObs = eObs.data(); g.eInvSigma2 = eInv.data();
    g.iKF1 = iKF1.data(); g.iKF2 = iKF2.data(); g.iPre = iPre.data();
    g.fx = k0->fx; g.fy = k0->fy; g.cx = k0->cx; g.cy = k0->cy; g.mbf = k0->mbf;
    float rigp[28];
    if (rig) {
      KF* kr = nullptr;
      for (KF* k : kfs) if (k->mpCamera2) { kr = k; break; }
      morb_glue::rig28(kr, rigp); g.rig28 = rigp; g.eRight = eRight.data();
    }
    FullInertialBA(g, its, bInit, priorG, priorA, pbStopFlag, pbStopFlag ? kLoopClosing : kMapping);
    if (g.stats[2] == 0 && pbStopFlag && *pbStopFlag) return;   // (the flag was raised between the check above and the entry's own)
  }
  // :696-740: Tcw = (Rcb Rwb^T, tcb - Rcb Rwb^T twb) (ImuCamPose, G2oTypes.cc:74-113), velocity, bias
  for (size_t i = 0; i < kfs.size(); ++i) {
    KF* pKFi = kfs[i];
    const float* s = &kfState[21 * i];
    const float* Tbc = g.Tbc12;
    double Rcw[9], tcw[3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) { double a = 0; for (int k = 0; k < 3; ++k) a += (double)Tbc[3 * k + r] * s[3 * c + k]; Rcw[3 * r + c] = a; }
    for (int r = 0; r < 3; ++r) {
      double a = 0;
      for (int k = 0; k < 3; ++k) a -= (double)Tbc[3 * k + r] * Tbc[9 + k];
      for (int c = 0; c < 3; ++c) a -= Rcw[3 * r + c] * s[9 + c];
      tcw[r] = a;
    }
    const SE3 T = se3_from_matrix<SE3>(Rcw, tcw);
    if (nLoopId == 0) pKFi->SetPose(T);
    else { pKFi->mTcwGBA = T; pKFi->mnBAGlobalForKF = nLoopId; }
    if (!pKFi->bImu) continue;
    typename std::decay<decltype(pKFi->GetVelocity())>::type vel;
    for (int k = 0; k < 3; ++k) vel(k) = s[12 + k];
    const float* bb = bInit ? g.bias6 : s + 15;                                         // (:719-729: with bInit the shared vertices, for every keyframe)
    const Bias b(bb[3], bb[4], bb[5], bb[0], bb[1], bb[2]);
    if (nLoopId == 0) { pKFi->SetVelocity(vel); pKFi->SetNewBias(b); }
    else { pKFi->mVwbGBA = vel; pKFi->mBiasGBA = b; }
  }
  for (size_t j = 0; j < vpMPs.size(); ++j) {                                           // :743-757
    if (!included[j]) continue;
    MP* pMP = vpMPs[j];
    typename std::decay<decltype(pMP->GetWorldPos())>::type X;
    for (int k = 0; k < 3; ++k) X(k) = mpPos[3 * j + k];
    if (nLoopId == 0) { pMP->SetWorldPos(X); pMP->UpdateNormalAndDepth(); }
    else { pMP->mPosGBA = X; pMP->mnBAGlobalForKF = nLoopId; }
  }
  pMap->IncreaseChangeIndex();                                                          // :759
}

template <class SE3>
SE3 Optimizer::se3_from_matrix(const double R[9], const double t[3]) {
  typename std::decay<decltype(std::declval<SE3>().rotationMatrix())>::type Rm;
  typename SE3::Point tv;
  for (int r = 0; r < 3; ++r) { tv(r) = (float)t[r]; for (int c = 0; c < 3; ++c) Rm(r, c) = (float)R[3 * r + c]; }
  return SE3(Rm, tv);
}

}  // namespace ORB_SLAM3
