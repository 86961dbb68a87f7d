// TwoViewReconstruction in its caller's form, written for this test against the mocks of tests/native/mock_ref and
// tests/native/mock_two_view: a pinhole camera that builds its K, constructs the reconstructor on first use with the defaults and
// forwards (vKeys1, vKeys2, vMatches12, T21, vP3D, vbTriangulated), as Pinhole::ReconstructWithTwoViews does, and a tracking step that
// calls it between the matcher and the map creation.  It compiles <=> the adapter accepts such a caller (tests/test_two_view_cpu.py).
#include <vector>

#include "two_view_mock.h"             // tests/native/mock_two_view
#include "TwoViewReconstruction.h"     // include/morb

namespace ORB_SLAM3 {

struct PinholeCheck : GeometricCamera {
  TwoViewReconstruction* tvr = nullptr;
  Eigen::Matrix3f toK_() {
    Eigen::Matrix3f K;
    K(0, 0) = mvParameters[0]; K(0, 1) = 0.f; K(0, 2) = mvParameters[2];
    K(1, 0) = 0.f; K(1, 1) = mvParameters[1]; K(1, 2) = mvParameters[3];
    K(2, 0) = 0.f; K(2, 1) = 0.f; K(2, 2) = 1.f;
    return K;
  }
  __attribute__((used)) bool ReconstructWithTwoViews(const std::vector<cv::KeyPoint>& vKeys1, const std::vector<cv::KeyPoint>& vKeys2,
                                                     const std::vector<int>& vMatches12, Sophus::SE3f& T21, std::vector<cv::Point3f>& vP3D,
                                                     std::vector<bool>& vbTriangulated) {
    if (!tvr) {
      Eigen::Matrix3f K = this->toK_();
      tvr = new TwoViewReconstruction(K);
    }
    return tvr->Reconstruct(vKeys1, vKeys2, vMatches12, T21, vP3D, vbTriangulated);
  }
};

struct InitializationCheck {
  PinholeCheck* mpCamera = nullptr;
  std::vector<cv::KeyPoint> mvKeysUn1, mvKeysUn2;
  std::vector<int> mvIniMatches;
  std::vector<cv::Point3f> mvIniP3D;
  __attribute__((used)) int Step() {
    Sophus::SE3f Tcw;
    std::vector<bool> vbTriangulated;
    int n = 0;
    if (mpCamera->ReconstructWithTwoViews(mvKeysUn1, mvKeysUn2, mvIniMatches, Tcw, mvIniP3D, vbTriangulated))
      for (size_t i = 0; i < mvIniMatches.size(); ++i)
        if (mvIniMatches[i] >= 0 && !vbTriangulated[i]) { mvIniMatches[i] = -1; ++n; }
    TwoViewReconstruction other(mpCamera->toK_(), 2.0f, 100);   // the three-argument constructor
    TwoViewView v;
    return n + (other.Reconstruct(v) ? 1 : 0) + (int)Tcw.translation()(0);
  }
};
}  // namespace ORB_SLAM3
