// MOCKS — NOT the reference.  The names Optimizer::FullInertialBA(pMap, its, bFixLocal, nLoopId, pbStopFlag, bInit, priorG, priorA) of
// include/morb/Optimizer_reference.h touches, on the value types of tests/native/mock_ref/mock_types.h: a keyframe with its temporal
// predecessor, IMU state and preintegration, the two local-BA marks, both cameras' keypoints and the GBA members; a map point with its
// observations and GBA members; a map with its keyframes, points, largest keyframe id and change index.  Canned behaviour only: SetNewBias on a
// preintegration counts its calls, the setters count theirs.
#pragma once
#include <map>
#include <tuple>
#include <vector>

#include "../mock_sim3/g2o_sim3_mock.h"

namespace ORB_SLAM3 {

struct FIKeyFrame;
struct FIPreintegrated : IMU::Preintegrated {
  int nSetNewBias = 0; IMU::Bias last;
  void SetNewBias(const IMU::Bias& b_) { ++nSetNewBias; last = b_; }
};
struct FIMapPoint {
  long unsigned int mnId = 0, mnBAGlobalForKF = 0;
  Eigen::Vector3f mWorldPos, mPosGBA;
  std::map<FIKeyFrame*, std::tuple<int, int>> mObservations;
  int nSetPos = 0, nUpdates = 0;
  Eigen::Vector3f GetWorldPos() { return mWorldPos; }
  void SetWorldPos(const Eigen::Vector3f& p) { mWorldPos = p; ++nSetPos; }
  void UpdateNormalAndDepth() { ++nUpdates; }
  std::map<FIKeyFrame*, std::tuple<int, int>> GetObservations() { return mObservations; }
};
struct FIKeyFrame {
  long unsigned int mnId = 0, mnBALocalForKF = 0, mnBAFixedForKF = 0, mnBAGlobalForKF = 0;
  FIKeyFrame* mPrevKF = nullptr;
  bool bImu = true, mbBad = false;
  FIPreintegrated* mpImuPreintegrated = nullptr;
  IMU::Calib mImuCalib;
  GeometricCamera *mpCamera = nullptr, *mpCamera2 = nullptr;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  int NLeft = -1;
  std::vector<cv::KeyPoint> mvKeysUn, mvKeysRight;
  std::vector<float> mvuRight, mvInvLevelSigma2;
  Sophus::SE3f mTcw, mTrl, mTcwGBA;
  Eigen::Matrix3f mRwb; Eigen::Vector3f mOwb, mVw, mVwbGBA; IMU::Bias mImuBias, mBiasGBA;
  int nSetPose = 0, nSetVelocity = 0, nSetNewBias = 0;
  bool isBad() { return mbBad; }
  Sophus::SE3f GetPose() { return mTcw; }
  Sophus::SE3f GetRelativePoseTrl() { return mTrl; }
  void SetPose(const Sophus::SE3f& T) { mTcw = T; ++nSetPose; }
  Eigen::Matrix3f GetImuRotation() { return mRwb; }
  Eigen::Vector3f GetImuPosition() { return mOwb; }
  Eigen::Vector3f GetVelocity() { return mVw; }
  IMU::Bias GetImuBias() { return mImuBias; }
  void SetVelocity(const Eigen::Vector3f& v) { mVw = v; ++nSetVelocity; }
  void SetNewBias(const IMU::Bias& b) { mImuBias = b; ++nSetNewBias; }
};
struct FIMap {
  std::vector<FIKeyFrame*> kfs;
  std::vector<FIMapPoint*> mps;
  long unsigned int maxKFid = 0;
  int changes = 0;
  std::vector<FIKeyFrame*> GetAllKeyFrames() { return kfs; }
  std::vector<FIMapPoint*> GetAllMapPoints() { return mps; }
  long unsigned int GetMaxKFid() { return maxKFid; }
  void IncreaseChangeIndex() { ++changes; }
};
struct FIAtlas {
  FIMap* current = nullptr;
  FIMap* GetCurrentMap() { return current; }
};

}  // namespace ORB_SLAM3
