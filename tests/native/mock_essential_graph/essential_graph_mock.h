// MOCKS — NOT the reference, NOT g2o.  What Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3,
// LoopConnections, bFixScale) of include/morb/Optimizer_reference.h touches beyond the mocks of tests/native/mock_ref: the spanning tree, the loop
// edges and the covisibility lists of a keyframe, the correction marks of a map point, the map's lists, and a Sim3 with g2o::Sim3's
// interface (rotation(), translation(), scale(), operator*, inverse()) whose algebra is written here in FP64.
#pragma once
#include <map>
#include <set>
#include <vector>

#include "../mock_ref/KeyFrame.h"

namespace ORB_SLAM3 {

struct EGQuat {
  double v[4];   // x y z w
  EGQuat() : v{0, 0, 0, 1} {}
  EGQuat(double w, double x, double y, double z) : v{x, y, z, w} {}
  double x() const { return v[0]; } double y() const { return v[1]; } double z() const { return v[2]; } double w() const { return v[3]; }
};
struct EGVec3 { double v[3] = {0, 0, 0}; double operator()(int i) const { return v[i]; } double& operator()(int i) { return v[i]; } };
struct EGSim3 {
  EGQuat r; EGVec3 t; double s = 1;
  EGSim3() {}
  EGSim3(const EGQuat& q, const EGVec3& tt, double ss) : r(q), t(tt), s(ss) {}
  const EGQuat& rotation() const { return r; } const EGVec3& translation() const { return t; } double scale() const { return s; }
  static EGVec3 rot(const EGQuat& q, const EGVec3& x) {
    const double ux = q.v[0], uy = q.v[1], uz = q.v[2], w = q.v[3];
    double a = uy * x.v[2] - uz * x.v[1], b = uz * x.v[0] - ux * x.v[2], c = ux * x.v[1] - uy * x.v[0];
    a += a; b += b; c += c;
    EGVec3 o;
    o.v[0] = x.v[0] + w * a + (uy * c - uz * b); o.v[1] = x.v[1] + w * b + (uz * a - ux * c); o.v[2] = x.v[2] + w * c + (ux * b - uy * a);
    return o;
  }
  EGSim3 operator*(const EGSim3& o) const {
    EGSim3 m;
    const double *p = r.v, *q = o.r.v;
    m.r.v[3] = p[3] * q[3] - p[0] * q[0] - p[1] * q[1] - p[2] * q[2];
    m.r.v[0] = p[3] * q[0] + p[0] * q[3] + p[1] * q[2] - p[2] * q[1];
    m.r.v[1] = p[3] * q[1] + p[1] * q[3] + p[2] * q[0] - p[0] * q[2];
    m.r.v[2] = p[3] * q[2] + p[2] * q[3] + p[0] * q[1] - p[1] * q[0];
    const EGVec3 rt = rot(r, o.t);
    for (int k = 0; k < 3; ++k) m.t.v[k] = s * rt.v[k] + t.v[k];
    m.s = s * o.s;
    return m;
  }
  EGSim3 inverse() const {
    EGSim3 m;
    m.r = EGQuat(r.v[3], -r.v[0], -r.v[1], -r.v[2]);
    EGVec3 x;
    for (int k = 0; k < 3; ++k) x.v[k] = (-1. / s) * t.v[k];
    m.t = rot(m.r, x);
    m.s = 1. / s;
    return m;
  }
};

struct EGKeyFrame : KeyFrame {
  EGKeyFrame* parent = nullptr;
  std::set<EGKeyFrame*> children, loopEdges;
  std::map<EGKeyFrame*, int> weights;
  std::vector<EGKeyFrame*> covisibles;   // by descending weight, as GetCovisiblesByWeight hands them out
  int nSetPose = 0;
  EGKeyFrame* GetParent() { return parent; }
  bool hasChild(EGKeyFrame* k) { return children.count(k) != 0; }
  std::set<EGKeyFrame*> GetLoopEdges() { return loopEdges; }
  int GetWeight(EGKeyFrame* k) { return weights.count(k) ? weights[k] : 0; }
  std::vector<EGKeyFrame*> GetCovisiblesByWeight(const int& w) {
    std::vector<EGKeyFrame*> o;
    for (auto* k : covisibles) if (GetWeight(k) >= w) o.push_back(k);
    return o;
  }
  void SetPose(const Sophus::SE3f& T) { mTcw = T; ++nSetPose; }
};
struct EGMapPoint : MapPoint {
  long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
  EGKeyFrame* ref = nullptr;
  int nSetPos = 0;
  EGKeyFrame* GetReferenceKeyFrame() { return ref; }
  void SetWorldPos(const Eigen::Vector3f& p) { mWorldPos = p; ++nSetPos; }
};
struct EGMap : Map {
  std::vector<EGKeyFrame*> kfs; std::vector<EGMapPoint*> mps;
  std::vector<EGKeyFrame*> GetAllKeyFrames() { return kfs; }
  std::vector<EGMapPoint*> GetAllMapPoints() { return mps; }
  long unsigned int GetMaxKFid() { long unsigned int m = 0; for (auto* k : kfs) if (k->mnId > m) m = k->mnId; return m; }
};

}  // namespace ORB_SLAM3
