// Sim3Solver in the reference's call form: LoopClosing.cc:700-722 pasted verbatim into a member of a mock loop closer, compiled against
// the mocks of tests/native/mock_ref and tests/native/mock_sim3_solver.  It compiles <=> the adapter class accepts a loop-closing
// caller's code unchanged; the enclosing function is marked `used`, so every member is instantiated (tests/test_sim3_solver_cpu.py).
#include <vector>

#include "KeyFrame.h"   // tests/native/mock_ref
#include "Map.h"
#include "MapPoint.h"
#include "loop_closing_mock.h"   // tests/native/mock_sim3_solver
#include "Sim3Solver.h"          // include/morb

namespace ORB_SLAM3 {
std::mutex MapPoint::mGlobalMutex;

struct LoopClosingCheck {
  KeyFrame* mpCurrentKF = nullptr;
  TrackingMock* mpTracker = nullptr;
  bool mbFixScale = false;

  __attribute__((used)) int DetectFromBoW(KeyFrame* pMostBoWMatchesKF, std::vector<MapPoint*>& vpMatchedPoints,
                                          std::vector<KeyFrame*>& vpKeyFrameMatchedMP, int nBoWInliers) {
    // ---- LoopClosing.cc:700-722, verbatim ----
      bool bFixedScale = mbFixScale;
      if (mpTracker->mSensor == CameraType::IMU_MONOCULAR &&
          !mpCurrentKF->GetMap()->GetIniertialBA2())
        bFixedScale = false;

      Sim3Solver solver =
          Sim3Solver(mpCurrentKF, pMostBoWMatchesKF, vpMatchedPoints,
                     bFixedScale, vpKeyFrameMatchedMP);
      solver.SetRansacParameters(0.99, nBoWInliers,
                                 300);  // at least 15 inliers

      bool bNoMore = false;
      vector<bool> vbInliers;
      int nInliers;
      bool bConverge = false;
      Eigen::Matrix4f mTcm;
      while (!bConverge && !bNoMore) {
        mTcm = solver.iterate(20, bNoMore, vbInliers, nInliers, bConverge);
        // Verbose::PrintMess("BoW guess: Solver achieve " + to_string(nInliers)
        // + " geometrical inliers among " + to_string(nBoWInliers) + " BoW
        // matches", Verbose::VERBOSITY_DEBUG);
      }
    // ---- end of the verbatim block ----
    // the other members: find, the four-argument iterate, the getters, the default constructor arguments
    Sim3Solver s2(mpCurrentKF, pMostBoWMatchesKF, vpMatchedPoints);
    std::vector<bool> vb;
    int n2 = 0;
    Eigen::Matrix4f T = s2.find(vb, n2);
    T = s2.iterate(5, bNoMore, vb, n2);
    Eigen::Matrix4f Te = s2.GetEstimatedTransformation();
    Eigen::Matrix3f R = s2.GetEstimatedRotation();
    Eigen::Vector3f t = s2.GetEstimatedTranslation();
    const float s = s2.GetEstimatedScale();
    return nInliers + n2 + (int)(mTcm(0, 0) + T(0, 0) + Te(0, 0) + R(0, 0) + t(0) + s);
  }
};
}  // namespace ORB_SLAM3
