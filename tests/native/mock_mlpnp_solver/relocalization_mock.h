// MOCKS — NOT Eigen, NOT the reference.  What a relocalisation caller touches around the MLPnPsolver beyond tests/native/mock_ref:
// Eigen::Matrix4f.
#pragma once
#include "mock_types.h"

namespace Eigen {
typedef MatF<4, 4> Matrix4f;
}  // namespace Eigen
