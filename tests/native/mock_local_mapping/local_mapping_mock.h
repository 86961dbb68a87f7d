// MOCKS — NOT the reference.  What include/morb/LocalMapping.h touches beyond the mocks of tests/native/mock_ref: a KeyFrame with mvDepth,
// the covisibility list and the scene's median depth; a MapPoint that can be made from a position and counts its two updates; an Atlas
// that keeps what it is given; a Tracker with a state.  Canned behaviour only, as in mock_ref/mock_types.h.
#pragma once
#include <vector>

#include "KeyFrame.h"   // tests/native/mock_ref

namespace ORB_SLAM3 {

struct LMKeyFrame : KeyFrame {
  std::vector<float> mvDepth;
  std::vector<LMKeyFrame*> mvpBest;
  LMKeyFrame* mPrevKF = nullptr;   // (hides the base's: the adapter walks the chain in its own keyframe type)
  float medianDepth = 1.f;
  std::vector<LMKeyFrame*> GetBestCovisibilityKeyFrames(const int& n) {
    return std::vector<LMKeyFrame*>(mvpBest.begin(), mvpBest.begin() + std::min<size_t>((size_t)n, mvpBest.size()));
  }
  float ComputeSceneMedianDepth(const int) { return medianDepth; }
};

struct LMMapPoint : MapPoint {
  LMMapPoint(const Eigen::Vector3f& Pos, KeyFrame* pRefKF, Map* pMap) : mpRefKF(pRefKF) {
    mWorldPos = Pos; mpMap = pMap;
    mDescriptor.data.assign(32, 0); mDescriptor.rows = 1;   // (the next neighbour's search reads GetDescriptor() of every point a keyframe holds)
  }
  void ComputeDistinctiveDescriptors() { ++nDescriptorUpdates; }
  KeyFrame* mpRefKF;
  int nDescriptorUpdates = 0;
};

struct LMAtlas {
  Map map;
  std::vector<MapPoint*> points;
  Map* GetCurrentMap() { return &map; }
  void AddMapPoint(MapPoint* p) { points.push_back(p); }
};

struct LMTracker {
  enum eTrackingState { OK = 2, RECENTLY_LOST = 3 };
  eTrackingState mState = OK;
};

}  // namespace ORB_SLAM3
