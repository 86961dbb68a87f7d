// MOCKS — NOT the reference.  What the three Optimizer::InertialOptimization members of include/morb/Optimizer_reference.h touch beyond the
// mocks of tests/native/mock_ref: a Map that lists its keyframes and knows its largest keyframe id, a preintegration that counts its
// Reintegrate() calls, a keyframe whose mPrevKF and mpImuPreintegrated are of these types.  Canned behaviour only, as in mock_ref/mock_types.h.
#pragma once
#include <vector>

#include "../mock_ref/KeyFrame.h"

namespace ORB_SLAM3 {

struct IOPreintegrated : IMU::Preintegrated {
  int nReintegrated = 0, nSetNewBias = 0;
  void Reintegrate() { ++nReintegrated; }
  void SetNewBias(const IMU::Bias&) { ++nSetNewBias; }
};

struct IOKeyFrame : KeyFrame {
  IOKeyFrame* mPrevKF = nullptr;                 // (hide the base's: the adapter walks the chain in its own keyframe type)
  IOPreintegrated* mpImuPreintegrated = nullptr;
  Eigen::Vector3f GetGyroBias() { return Eigen::Vector3f(mImuBias.bwx, mImuBias.bwy, mImuBias.bwz); }
};

struct IOMap : Map {
  std::vector<IOKeyFrame*> keyframes;
  long unsigned int maxKFid = 0;
  std::vector<IOKeyFrame*> GetAllKeyFrames() { return keyframes; }
  long unsigned int GetMaxKFid() { return maxKFid; }
};

struct MatrixXd {};   // Eigen::MatrixXd covInertial: passed through, never read

}  // namespace ORB_SLAM3
