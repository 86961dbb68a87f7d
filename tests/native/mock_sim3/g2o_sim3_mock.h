// MOCKS — NOT Eigen, NOT g2o.  The names Optimizer::OptimizeSim3's reference-typed member touches beyond tests/native/mock_ref:
// Eigen::Quaterniond (x / y / z / w, (w, x, y, z) constructor), Eigen::Matrix<double, 7, 7> (setZero) and g2o::Sim3 (rotation,
// translation, scale, the (Quaterniond, Vector3d, double) constructor), as the reference headers declare them.
#pragma once
#include "mock_types.h"

namespace Eigen {
struct Quaterniond {
  double c[4];   // x y z w
  Quaterniond() : c{0, 0, 0, 1} {}
  Quaterniond(double w, double x, double y, double z) : c{x, y, z, w} {}
  double x() const { return c[0]; } double y() const { return c[1]; } double z() const { return c[2]; } double w() const { return c[3]; }
};
template <class S, int R, int C> struct Matrix {
  S m[R * C];
  void setZero() { for (S& v : m) v = 0; }
  S operator()(int r, int c) const { return m[C * r + c]; }
};
}  // namespace Eigen

namespace g2o {
struct Sim3 {
  Eigen::Quaterniond r;
  Eigen::Vector3d t;
  double s = 1.;
  Sim3() {}
  Sim3(const Eigen::Quaterniond& r_, const Eigen::Vector3d& t_, double s_) : r(r_), t(t_), s(s_) {}
  const Eigen::Quaterniond& rotation() const { return r; }
  const Eigen::Vector3d& translation() const { return t; }
  const double& scale() const { return s; }
};
}  // namespace g2o
