// MOCKS — NOT Eigen, NOT the reference.  What LoopClosing.cc:700-722 touches around the Sim3Solver beyond tests/native/mock_ref:
// Eigen::Matrix4f, the tracker's sensor, CameraType and Map::GetIniertialBA2, as the reference headers declare them.
#pragma once
#include "mock_types.h"

namespace Eigen {
typedef MatF<4, 4> Matrix4f;
}  // namespace Eigen

namespace ORB_SLAM3 {
struct CameraType { enum eSensor { MONOCULAR = 0, STEREO = 1, RGBD = 2, IMU_MONOCULAR = 3, IMU_STEREO = 4, IMU_RGBD = 5 }; };
struct TrackingMock { int mSensor = CameraType::MONOCULAR; };
using std::vector;   // the reference headers bring std into scope (`using namespace std`)
}  // namespace ORB_SLAM3
