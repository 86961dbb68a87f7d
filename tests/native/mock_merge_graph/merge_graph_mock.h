// MOCKS — NOT the reference, NOT Sophus.  What Optimizer::OptimizeEssentialGraph(pCurKF, vpFixedKFs, vpFixedCorrectedKFs, vpNonFixedKFs,
// vpNonCorrectedMPs) of include/morb/Optimizer_reference.h touches: a keyframe's pose and its two BefMerge members, its spanning tree, loop
// edges and covisibility list, a point's reference keyframe and observations, the map's largest keyframe id and its update mutex.  The SE3
// stores the quaternion and the translation it is given, bit for bit; its inverse is computed in float.
#pragma once
#include <cmath>
#include <map>
#include <mutex>
#include <set>
#include <vector>

namespace ORB_SLAM3 {

struct MGVec3 {
  float v[3] = {0, 0, 0};
  MGVec3() {}
  MGVec3(float a, float b, float c) : v{a, b, c} {}
  float operator()(int i) const { return v[i]; }
  float& operator()(int i) { return v[i]; }
};
struct MGQuat {
  float q[4] = {0, 0, 0, 1};   // x y z w
  MGQuat() {}
  MGQuat(float w, float x, float y, float z) : q{x, y, z, w} {}
  float x() const { return q[0]; } float y() const { return q[1]; } float z() const { return q[2]; } float w() const { return q[3]; }
};
struct MGSE3 {
  using QuaternionType = MGQuat;
  using Point = MGVec3;
  MGQuat q; MGVec3 t;
  MGSE3() {}
  MGSE3(const MGQuat& qq, const MGVec3& tt) : q(qq), t(tt) {}
  MGQuat unit_quaternion() const { return q; }
  MGVec3 translation() const { return t; }
  MGSE3 inverse() const {
    MGSE3 o;
    o.q = MGQuat(q.q[3], -q.q[0], -q.q[1], -q.q[2]);
    const float *u = o.q.q, m[3] = {-t.v[0], -t.v[1], -t.v[2]};
    float a = u[1] * m[2] - u[2] * m[1], b = u[2] * m[0] - u[0] * m[2], c = u[0] * m[1] - u[1] * m[0];
    a += a; b += b; c += c;
    o.t = MGVec3(m[0] + u[3] * a + (u[1] * c - u[2] * b), m[1] + u[3] * b + (u[2] * a - u[0] * c), m[2] + u[3] * c + (u[0] * b - u[1] * a));
    return o;
  }
};

struct MGKeyFrame;
struct MGMap {
  std::mutex mMutexMapUpdate;
  long unsigned int maxKFid = 0;
  long unsigned int GetMaxKFid() { return maxKFid; }
};
struct MGKeyFrame {
  long unsigned int mnId = 0;
  MGSE3 mTcw, mTwc, mTcwBefMerge, mTwcBefMerge;
  bool mbBad = false;
  MGMap* mpMap = nullptr;
  MGKeyFrame* parent = nullptr;
  std::set<MGKeyFrame*> children, loopEdges;
  std::vector<std::pair<MGKeyFrame*, int>> covisibles;   // (keyframe, weight) by descending weight
  int nSetPose = 0;
  bool isBad() { return mbBad; }
  MGMap* GetMap() { return mpMap; }
  MGSE3 GetPose() { return mTcw; }
  MGSE3 GetPoseInverse() { return mTwc; }
  void SetPose(const MGSE3& T) { mTcw = T; mTwc = T.inverse(); ++nSetPose; }
  MGKeyFrame* GetParent() { return parent; }
  bool hasChild(MGKeyFrame* k) { return children.count(k) != 0; }
  std::set<MGKeyFrame*> GetLoopEdges() { return loopEdges; }
  std::vector<MGKeyFrame*> GetCovisiblesByWeight(const int& w) {
    std::vector<MGKeyFrame*> o;
    for (auto& kw : covisibles) if (kw.second >= w) o.push_back(kw.first);
    return o;
  }
};
struct MGMapPoint {
  long unsigned int mnId = 0;
  MGVec3 mWorldPos;
  bool mbBad = false;
  std::vector<MGKeyFrame*> observers;   // the reference keyframe is the first observer left
  int nSetPos = 0, nUpdates = 0, nErased = 0;
  bool isBad() { return mbBad; }
  MGKeyFrame* GetReferenceKeyFrame() { return observers.empty() ? nullptr : observers.front(); }
  void EraseObservation(MGKeyFrame* k) {
    for (size_t i = 0; i < observers.size(); ++i) if (observers[i] == k) { observers.erase(observers.begin() + i); ++nErased; return; }
  }
  MGVec3 GetWorldPos() { return mWorldPos; }
  void SetWorldPos(const MGVec3& p) { mWorldPos = p; ++nSetPos; }
  void UpdateNormalAndDepth() { ++nUpdates; }
};

}  // namespace ORB_SLAM3
