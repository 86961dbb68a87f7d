// MOCKS — NOT the reference.  What Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag) of
// include/morb/Optimizer_reference.h touches beyond the mocks of tests/native/mock_ref: the merge mark of a keyframe and of a map point
// (mnBALocalForMerge), and getters that hand out the derived types.  Canned behaviour only, as in mock_ref/mock_types.h: an SE3f carries the
// quaternion and the translation it was given.
#pragma once
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "../mock_ref/KeyFrame.h"

namespace ORB_SLAM3 {

struct MBKeyFrame;
struct MBMap : Map {};

struct MBMapPoint : MapPoint {
  long unsigned int mnBALocalForMerge = 0;
  MBMap* GetMap() { return static_cast<MBMap*>(mpMap); }
  inline std::map<MBKeyFrame*, std::tuple<int, int>> GetObservations();
  void AddObservation(KeyFrame* k, int left, int right) { mObservations[k] = std::make_tuple(left, right); ++nObs; }
  int nSetPos = 0;
  void SetWorldPos(const Eigen::Vector3f& p) { mWorldPos = p; ++nSetPos; }
};

struct MBKeyFrame : KeyFrame {
  long unsigned int mnBALocalForMerge = 0;
  int nSetPose = 0;
  MBMap* GetMap() { return static_cast<MBMap*>(mpMap); }
  void SetPose(const Sophus::SE3f& T) { mTcw = T; ++nSetPose; }
  MBMapPoint* GetMapPoint(const size_t& idx) { return static_cast<MBMapPoint*>(mvpMapPoints[idx]); }
  std::set<MBMapPoint*> GetMapPoints() {
    std::set<MBMapPoint*> s;
    for (auto* p : mvpMapPoints) if (p && !p->isBad()) s.insert(static_cast<MBMapPoint*>(p));
    return s;
  }
};

inline std::map<MBKeyFrame*, std::tuple<int, int>> MBMapPoint::GetObservations() {
  std::map<MBKeyFrame*, std::tuple<int, int>> o;
  for (const auto& kv : mObservations) o[static_cast<MBKeyFrame*>(kv.first)] = kv.second;
  return o;
}

}  // namespace ORB_SLAM3
