// The call expression of LoopClosing::MergeLocal (src/LoopClosing.cc:1747-1749), unedited, against the mocks of
// tests/native/mock_merge_graph: it must pick the reference-typed member of overload 2 (include/morb/Optimizer_reference.h) and
// instantiate it.  Compiled only (tests/test_merge_graph_cpu.py); tests/native/merge_graph_member_check.cc runs the member.
#include <vector>

#include "merge_graph_mock.h"
#include "Optimizer.h"

using namespace ORB_SLAM3;
using std::vector;
typedef MGKeyFrame KeyFrame;
typedef MGMapPoint MapPoint;

struct CameraType { enum Sensor { MONOCULAR, STEREO }; };
struct TrackerLike { int mSensor = CameraType::STEREO; };

struct LoopClosingLike {
  TrackerLike* mpTracker;
  KeyFrame* mpCurrentKF;
  void MergeLocal();
};

void LoopClosingLike::MergeLocal() {
  vector<KeyFrame*> vpMergeConnectedKFs, vpLocalCurrentWindowKFs, vpCurrentMapKFs;
  vector<MapPoint*> vpCurrentMapMPs;
    if (mpTracker->mSensor != CameraType::MONOCULAR) {
      Optimizer::OptimizeEssentialGraph(mpCurrentKF, vpMergeConnectedKFs,
                                        vpLocalCurrentWindowKFs,
                                        vpCurrentMapKFs, vpCurrentMapMPs);
    }
}
