// Optimizer::OptimizeSim3 in the reference's call form (the signature of include/Optimizer.h:97-101: KeyFrame*, KeyFrame*,
// vector<MapPoint*>&, g2o::Sim3&, float th2, bool bFixScale, Eigen::Matrix<double, 7, 7>&, bool bAllPoints) compiled against the mocks of
// tests/native/mock_ref and tests/native/mock_sim3.  It compiles <=> the member template accepts a loop-closing caller's arguments unchanged;
// the enclosing function is marked `used`, so the member is instantiated (tests/test_sim3_cpu.py checks the symbol).
#include <vector>

#include "KeyFrame.h"      // tests/native/mock_ref
#include "MapPoint.h"
#include "g2o_sim3_mock.h"  // tests/native/mock_sim3
#include "Optimizer.h"      // include/morb

namespace ORB_SLAM3 {
std::mutex MapPoint::mGlobalMutex;

struct LoopCandidateCheck {
  KeyFrame* mpCurrentKF = nullptr;
  bool mbFixScale = false;

  __attribute__((used)) int RefineCandidate(KeyFrame* pKFi, std::vector<MapPoint*>& vpMatchedMPs, g2o::Sim3& gScm) {
    Eigen::Matrix<double, 7, 7> mHessian7x7;
    const bool bFixedScale = mbFixScale;
    const int numOptMatches = Optimizer::OptimizeSim3(mpCurrentKF, pKFi, vpMatchedMPs, gScm, 10, bFixedScale, mHessian7x7, true);
    const int numDefault = Optimizer::OptimizeSim3(mpCurrentKF, pKFi, vpMatchedMPs, gScm, 10, bFixedScale, mHessian7x7);   // bAllPoints = false
    return numOptMatches + numDefault;
  }
};
}  // namespace ORB_SLAM3
