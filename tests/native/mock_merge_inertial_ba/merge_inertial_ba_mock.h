// MOCKS — NOT the reference.  The names Optimizer::MergeInertialBA(pCurrKF, pMergeKF, pbStopFlag, pMap, corrPoses) of
// include/morb/Optimizer_reference.h touches, on the value types of tests/native/mock_ref/mock_types.h and the g2o::Sim3 of
// tests/native/mock_sim3: a keyframe with both temporal neighbours (mPrevKF, mNextKF), its IMU state and preintegration, the two marks
// (mnBALocalForKF, mnBAFixedForKF); a map point with its observations; a map with the update mutex.  Canned behaviour only: an SE3f built from
// a rotation matrix keeps the identity quaternion, SetNewBias on a preintegration counts its calls.  A keyframe and a map point note the order in
// which the member first read their state (readOrder, -1: never): the member reads them in the order of its vertices and of its points.
#pragma once
#include <map>
#include <tuple>
#include <vector>

#include "../mock_sim3/g2o_sim3_mock.h"

namespace ORB_SLAM3 {

struct MIKeyFrame;
inline int& mi_read_counter() { static int n = 0; return n; }
struct MIPreintegrated : IMU::Preintegrated {
  int nSetNewBias = 0; IMU::Bias last;
  void SetNewBias(const IMU::Bias& b_) { ++nSetNewBias; last = b_; }
};
struct MIMap {
  std::mutex mMutexMapUpdate;
  int changes = 0;
  void IncreaseChangeIndex() { ++changes; }
};
struct MIMapPoint {
  long unsigned int mnId = 0, mnBALocalForKF = 0;
  bool mbBad = false;
  Eigen::Vector3f mWorldPos;
  std::map<MIKeyFrame*, std::tuple<int, int>> mObservations;
  int nSetPos = 0, nUpdates = 0;
  bool isBad() { return mbBad; }
  int readOrder = -1;
  Eigen::Vector3f GetWorldPos() { if (readOrder < 0) readOrder = mi_read_counter()++; return mWorldPos; }
  void SetWorldPos(const Eigen::Vector3f& p) { mWorldPos = p; ++nSetPos; }
  void UpdateNormalAndDepth() { ++nUpdates; }
  std::map<MIKeyFrame*, std::tuple<int, int>> GetObservations() { return mObservations; }
  void EraseObservation(MIKeyFrame* k) { mObservations.erase(k); }
};
struct MIKeyFrame {
  long unsigned int mnId = 0, mnBALocalForKF = 0, mnBAFixedForKF = 0;
  MIKeyFrame *mPrevKF = nullptr, *mNextKF = nullptr;
  bool bImu = true, mbBad = false;
  MIPreintegrated* mpImuPreintegrated = nullptr;
  IMU::Calib mImuCalib;
  GeometricCamera *mpCamera = nullptr, *mpCamera2 = nullptr;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvuRight, mvInvLevelSigma2;
  std::vector<MIMapPoint*> mvpMapPoints;
  Sophus::SE3f mTcw, mTrl;
  Eigen::Matrix3f mRwb; Eigen::Vector3f mOwb, mVw; IMU::Bias mImuBias;
  int nSetPose = 0, nSetVelocity = 0, nSetNewBias = 0;
  bool isBad() { return mbBad; }
  Sophus::SE3f GetPose() { return mTcw; }
  Sophus::SE3f GetRelativePoseTrl() { return mTrl; }
  void SetPose(const Sophus::SE3f& T) { mTcw = T; ++nSetPose; }
  std::vector<MIMapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  void EraseMapPointMatch(MIMapPoint* p) { for (auto& q : mvpMapPoints) if (q == p) q = nullptr; }
  int readOrder = -1;
  Eigen::Matrix3f GetImuRotation() { if (readOrder < 0) readOrder = mi_read_counter()++; return mRwb; }
  Eigen::Vector3f GetImuPosition() { return mOwb; }
  Eigen::Vector3f GetVelocity() { return mVw; }
  IMU::Bias GetImuBias() { return mImuBias; }
  void SetVelocity(const Eigen::Vector3f& v) { mVw = v; ++nSetVelocity; }
  void SetNewBias(const IMU::Bias& b) { mImuBias = b; ++nSetNewBias; }
};

}  // namespace ORB_SLAM3
