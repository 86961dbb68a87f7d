// MOCKS — NOT the reference, NOT g2o.  What Optimizer::OptimizeEssentialGraph4DoF(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3,
// LoopConnections) of include/morb/Optimizer_reference.h touches beyond the mocks of tests/native/mock_ref: a keyframe's rotation, translation
// and IMU pose as float members, mNextKF, its children, loop edges and covisibility lists, mImuCalib.mTcb, the map's lists, and a Sim3 with
// g2o::Sim3's interface (rotation(), translation(), scale(), operator*, inverse()) whose algebra is written here in FP64.
#pragma once
#include <map>
#include <set>
#include <vector>

#include "../mock_ref/KeyFrame.h"

namespace ORB_SLAM3 {

struct PGQuat {
  double v[4];   // x y z w
  PGQuat() : v{0, 0, 0, 1} {}
  PGQuat(double w, double x, double y, double z) : v{x, y, z, w} {}
  double x() const { return v[0]; } double y() const { return v[1]; } double z() const { return v[2]; } double w() const { return v[3]; }
};
struct PGVec3 { double v[3] = {0, 0, 0}; double operator()(int i) const { return v[i]; } double& operator()(int i) { return v[i]; } };
struct PGSim3 {
  PGQuat r; PGVec3 t; double s = 1;
  PGSim3() {}
  PGSim3(const PGQuat& q, const PGVec3& tt, double ss) : r(q), t(tt), s(ss) {}
  const PGQuat& rotation() const { return r; } const PGVec3& translation() const { return t; } double scale() const { return s; }
  static PGVec3 rot(const PGQuat& q, const PGVec3& x) {
    const double ux = q.v[0], uy = q.v[1], uz = q.v[2], w = q.v[3];
    double a = uy * x.v[2] - uz * x.v[1], b = uz * x.v[0] - ux * x.v[2], c = ux * x.v[1] - uy * x.v[0];
    a += a; b += b; c += c;
    PGVec3 o;
    o.v[0] = x.v[0] + w * a + (uy * c - uz * b); o.v[1] = x.v[1] + w * b + (uz * a - ux * c); o.v[2] = x.v[2] + w * c + (ux * b - uy * a);
    return o;
  }
  PGSim3 operator*(const PGSim3& o) const {
    PGSim3 m;
    const double *p = r.v, *q = o.r.v;
    m.r.v[3] = p[3] * q[3] - p[0] * q[0] - p[1] * q[1] - p[2] * q[2];
    m.r.v[0] = p[3] * q[0] + p[0] * q[3] + p[1] * q[2] - p[2] * q[1];
    m.r.v[1] = p[3] * q[1] + p[1] * q[3] + p[2] * q[0] - p[0] * q[2];
    m.r.v[2] = p[3] * q[2] + p[2] * q[3] + p[0] * q[1] - p[1] * q[0];
    const PGVec3 rt = rot(r, o.t);
    for (int k = 0; k < 3; ++k) m.t.v[k] = s * rt.v[k] + t.v[k];
    m.s = s * o.s;
    return m;
  }
  PGSim3 inverse() const {
    PGSim3 m;
    m.r = PGQuat(r.v[3], -r.v[0], -r.v[1], -r.v[2]);
    PGVec3 x;
    for (int k = 0; k < 3; ++k) x.v[k] = (-1. / s) * t.v[k];
    m.t = rot(m.r, x);
    m.s = 1. / s;
    return m;
  }
};

struct PGCalib { Sophus::SE3f mTcb; };
struct PGKeyFrame : KeyFrame {
  PGCalib mImuCalib;                     // (hides the base's, which has no mTcb)
  KeyFrame* mNextKF = nullptr;
  std::set<PGKeyFrame*> children, loopEdges;
  std::map<PGKeyFrame*, int> weights;
  std::vector<PGKeyFrame*> covisibles;   // by descending weight, as GetCovisiblesByWeight hands them out
  Eigen::Matrix3f mRcw; Eigen::Vector3f mtcw;
  int nSetPose = 0;
  Eigen::Matrix3f GetRotation() { return mRcw; }
  Eigen::Vector3f GetTranslation() { return mtcw; }
  bool hasChild(PGKeyFrame* k) { return children.count(k) != 0; }
  std::set<PGKeyFrame*> GetLoopEdges() { return loopEdges; }
  int GetWeight(PGKeyFrame* k) { return weights.count(k) ? weights[k] : 0; }
  std::vector<PGKeyFrame*> GetCovisiblesByWeight(const int& w) {
    std::vector<PGKeyFrame*> o;
    for (auto* k : covisibles) if (GetWeight(k) >= w) o.push_back(k);
    return o;
  }
  void SetPose(const Sophus::SE3f& T) { mTcw = T; ++nSetPose; }
};
struct PGMapPoint : MapPoint {
  PGKeyFrame* ref = nullptr;
  int nSetPos = 0;
  PGKeyFrame* GetReferenceKeyFrame() { return ref; }
  void SetWorldPos(const Eigen::Vector3f& p) { mWorldPos = p; ++nSetPos; }
};
struct PGMap : Map {
  std::vector<PGKeyFrame*> kfs; std::vector<PGMapPoint*> mps;
  std::vector<PGKeyFrame*> GetAllKeyFrames() { return kfs; }
  std::vector<PGMapPoint*> GetAllMapPoints() { return mps; }
  long unsigned int GetMaxKFid() { long unsigned int m = 0; for (auto* k : kfs) if (k->mnId > m) m = k->mnId; return m; }
};

}  // namespace ORB_SLAM3
