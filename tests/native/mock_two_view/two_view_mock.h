// MOCKS — NOT OpenCV, NOT the reference.  What a monocular-initialisation caller touches around TwoViewReconstruction beyond
// tests/native/mock_ref: cv::Point3f.
#pragma once
#include "mock_types.h"

namespace cv {
struct Point3f {
  float x = 0, y = 0, z = 0;
  Point3f() {}
  Point3f(float a, float b, float c) : x(a), y(b), z(c) {}
};
}  // namespace cv
