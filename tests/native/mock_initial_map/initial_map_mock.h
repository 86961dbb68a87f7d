// MOCKS — NOT the reference.  What Optimizer::GlobalBundleAdjustemnt / BundleAdjustment of include/morb/Optimizer_reference.h touch beyond the
// mocks of tests/native/mock_ref: a Map that lists its keyframes and points and knows its origin keyframe, and the GBA fields of a keyframe
// and of a map point.  Canned behaviour only, as in mock_ref/mock_types.h.
#pragma once
#include <vector>

#include "../mock_ref/KeyFrame.h"

namespace ORB_SLAM3 {

struct IMMap;
struct IMKeyFrame : KeyFrame {
  Sophus::SE3f mTcwGBA;
  long unsigned int mnBAGlobalForKF = 0;
  IMMap* GetMap();   // (hide the base's: the adapter asks the map for its origin keyframe)
};

struct IMMapPoint : MapPoint {
  Eigen::Vector3f mPosGBA;
  long unsigned int mnBAGlobalForKF = 0;
};

struct IMMap : Map {
  std::vector<IMKeyFrame*> keyframes;
  std::vector<IMMapPoint*> points;
  std::vector<IMKeyFrame*> GetAllKeyFrames() { return keyframes; }
  std::vector<IMMapPoint*> GetAllMapPoints() { return points; }
  IMKeyFrame* GetOriginKF() { return keyframes.front(); }
};

inline IMMap* IMKeyFrame::GetMap() { return static_cast<IMMap*>(mpMap); }

}  // namespace ORB_SLAM3
