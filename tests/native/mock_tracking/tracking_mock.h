// MOCKS — NOT the reference.  What Tracking::UpdateLocalMap touches of Frame, KeyFrame, MapPoint and Atlas, as the reference headers
// declare it, with plain members behind the accessors so that a test can build a map by hand.
#pragma once
#include <map>
#include <set>
#include <tuple>
#include <vector>

namespace ORB_SLAM3 {

class KeyFrame;

class MapPoint {
 public:
  bool isBad() { return mbBad; }
  std::map<KeyFrame*, std::tuple<int, int>> GetObservations() { return mObservations; }
  long unsigned int mnTrackReferenceForFrame = 0;
  // (mock state)
  bool mbBad = false;
  std::map<KeyFrame*, std::tuple<int, int>> mObservations;
};

class KeyFrame {
 public:
  bool isBad() { return mbBad; }
  std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
    return (int)mvpOrdered.size() < N ? mvpOrdered : std::vector<KeyFrame*>(mvpOrdered.begin(), mvpOrdered.begin() + N);
  }
  std::set<KeyFrame*> GetChilds() { return mspChildrens; }
  KeyFrame* GetParent() { return mpParent; }
  KeyFrame* mPrevKF = nullptr;
  long unsigned int mnTrackReferenceForFrame = 0;
  // (mock state)
  bool mbBad = false;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<KeyFrame*> mvpOrdered;
  std::set<KeyFrame*> mspChildrens;
  KeyFrame* mpParent = nullptr;
};

class Frame {
 public:
  long unsigned int mnId = 0;
  int N = 0;
  std::vector<MapPoint*> mvpMapPoints;
  KeyFrame* mpLastKeyFrame = nullptr;
  KeyFrame* mpReferenceKF = nullptr;
};

class Atlas {
 public:
  bool isImuInitialized() { return mbImuInitialized; }
  std::vector<KeyFrame*> GetAllKeyFrames() { return mvpKeyFrames; }
  std::vector<MapPoint*> GetAllMapPoints() { return mvpMapPoints; }
  void SetReferenceMapPoints(const std::vector<MapPoint*>& v) { mvpReferenceMapPoints = v; }
  // (mock state)
  bool mbImuInitialized = false;
  std::vector<KeyFrame*> mvpKeyFrames;
  std::vector<MapPoint*> mvpMapPoints, mvpReferenceMapPoints;
};

}  // namespace ORB_SLAM3
