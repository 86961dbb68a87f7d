// MOCKS — NOT the reference.  What Optimizer::WholeMapBundleAdjustment / BundleAdjustment / GlobalBundleAdjustemnt of
// include/morb/Optimizer_reference.h touch beyond the mocks of tests/native/mock_ref: a Map that lists its keyframes and points and knows its
// origin keyframe, the GBA fields of a keyframe and of a map point, getters that hand out the derived types, and counters of the
// write-backs.  Canned behaviour only, as in mock_ref/mock_types.h: an SE3f carries the quaternion and the translation it was given.
#pragma once
#include <map>
#include <tuple>
#include <vector>

#include "../mock_ref/KeyFrame.h"

namespace ORB_SLAM3 {

struct GBMap;
struct GBKeyFrame : KeyFrame {
  Sophus::SE3f mTcwGBA;
  long unsigned int mnBAGlobalForKF = 0;
  int nSetPose = 0;
  GBMap* GetMap();
  void SetPose(const Sophus::SE3f& T) { mTcw = T; ++nSetPose; }
};

struct GBMapPoint : MapPoint {
  Eigen::Vector3f mPosGBA;
  long unsigned int mnBAGlobalForKF = 0;
  int nSetPos = 0;
  std::map<GBKeyFrame*, std::tuple<int, int>> GetObservations() {
    std::map<GBKeyFrame*, std::tuple<int, int>> o;
    for (const auto& kv : mObservations) o[static_cast<GBKeyFrame*>(kv.first)] = kv.second;
    return o;
  }
  void AddObservation(KeyFrame* k, int left, int right) { mObservations[k] = std::make_tuple(left, right); ++nObs; }
  void SetWorldPos(const Eigen::Vector3f& p) { mWorldPos = p; ++nSetPos; }
};

struct GBMap : Map {
  std::vector<GBKeyFrame*> keyframes;
  std::vector<GBMapPoint*> points;
  GBKeyFrame* origin = nullptr;
  std::vector<GBKeyFrame*> GetAllKeyFrames() { return keyframes; }
  std::vector<GBMapPoint*> GetAllMapPoints() { return points; }
  GBKeyFrame* GetOriginKF() { return origin; }
};

inline GBMap* GBKeyFrame::GetMap() { return static_cast<GBMap*>(mpMap); }

}  // namespace ORB_SLAM3
