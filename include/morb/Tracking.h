// Tracking::UpdateLocalMap (reference src/Tracking.cc:3184-3358) with the reference's member names, over morb_update_local_map_batch.
//   UpdateLocalMap(LocalMapView&)  one query on flattened tables: the call a caller makes whose map tables it keeps itself;
//   UpdateLocalMap()               the reference's member: flattens the map reachable from mpAtlas, runs the view call and writes back
//                                  mvpLocalKeyFrames, mvpLocalMapPoints, both mnTrackReferenceForFrame stamps, the NULLed entries of the
//                                  voting frame, and mpReferenceKF on the tracker and on mCurrentFrame.
// A template on the caller's types, as the other adapters are.  What it touches:
//   Frame     mnId, N, mvpMapPoints, mpLastKeyFrame, mpReferenceKF;
//   KeyFrame  isBad, GetMapPointMatches, GetBestCovisibilityKeyFrames, GetChilds, GetParent, mPrevKF, mnTrackReferenceForFrame;
//   MapPoint  isBad, GetObservations (a map keyed by KeyFrame*), mnTrackReferenceForFrame;
//   Atlas     isImuInitialized, GetAllKeyFrames, GetAllMapPoints, SetReferenceMapPoints.
// Rows: the keyframes and points of the atlas' current map in the order it returns them, then whatever else the graph reaches (a
// parent, a neighbour, an observer, a frame's point that the map no longer lists).  d_kfOrder is each keyframe's rank under
// std::less<KeyFrame*>: the order in which std::map<KeyFrame*, int> (:3222) and std::set<KeyFrame*> (GetChilds) iterate.
// The member flattens the WHOLE map on every call, which costs the host what the reference's loop costs and more; it exists so that the
// reference's call compiles and can be tested.  A tracker that keeps the tables resident calls the entry point (or the view call) with
// only the frame's table changing from frame to frame.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "device_buffer.h"
#include "local_map_math.h"
#include "morb_hip.h"

namespace ORB_SLAM3 {

// the tables of morb_update_local_map_batch for one query, on the host
struct LocalMapView {
  int nkf = 0, kfCap = 1, ncovis = 0, nmp = 0;
  std::vector<int> kfMp, kfCount, kfOrder, covis, childStart, child, parent, prevKf, mpObsStart, mpObsKf;
  std::vector<uint8_t> kfFlags, mpFlags;
  std::vector<int> frameMp;   // in / out
  int lastKf = -1;
  bool inertial = false;
  // results
  std::vector<int> localKf, localMp, frameLocal, votes;
  int refKf = -1;
};

template <class Frame, class KeyFrame, class MapPoint, class Atlas>
class TrackingT {
 public:
  // include/Tracking.h
  Frame mCurrentFrame, mLastFrame;
  std::vector<KeyFrame*> mvpLocalKeyFrames;
  std::vector<MapPoint*> mvpLocalMapPoints;
  KeyFrame* mpReferenceKF = nullptr;
  unsigned int mnLastRelocFrameId = 0;
  Atlas* mpAtlas = nullptr;
  int mSensor = 0;   // CameraType::eSensor (include/ImprovedTypes.hpp:39-46): IMU_MONOCULAR = 3, IMU_STEREO = 4, IMU_RGBD = 5

  explicit TrackingT(int device = 0) : device_(device) {}
  ~TrackingT() { if (h_) morb_matcher_destroy(h_); }
  TrackingT(const TrackingT&) = delete;
  TrackingT& operator=(const TrackingT&) = delete;

  static bool IsInertial(int sensor) { return sensor == 3 || sensor == 4 || sensor == 5; }

  // The rows the last Flatten / UpdateLocalMap() gave out.
  std::vector<KeyFrame*> rowKF;
  std::vector<MapPoint*> rowMP;

  void UpdateLocalMap(LocalMapView& v) {
    if (!h_ && morb_matcher_create(&h_, device_) != MORB_OK) throw std::runtime_error(std::string("morb_matcher_create: ") + morb_last_error());
    const int cap = std::max<int>((int)v.frameMp.size(), 1), kfOut = std::max(v.nkf, 1), mpCap = std::max(v.nmp, 1);   // both lists are duplicate-free
    const int count = (int)v.frameMp.size();
    morb_adapter::CallStaging c(device_, morb_matcher_stream(h_));
    const int* d_kfMp = c.in(v.kfMp.data(), v.kfMp.size());
    const int* d_kfCount = c.in(v.kfCount.data(), v.kfCount.size());
    const uint8_t* d_kfFlags = c.in(v.kfFlags.data(), v.kfFlags.size());
    const int* d_kfOrder = v.kfOrder.empty() ? nullptr : c.in(v.kfOrder.data(), v.kfOrder.size());
    const int* d_covis = c.in(v.covis.data(), v.covis.size());
    const int* d_childStart = v.childStart.empty() ? nullptr : c.in(v.childStart.data(), v.childStart.size());
    const int* d_child = c.in(v.child.data(), v.child.size());
    const int* d_parent = v.parent.empty() ? nullptr : c.in(v.parent.data(), v.parent.size());
    const int* d_prevKf = v.prevKf.empty() ? nullptr : c.in(v.prevKf.data(), v.prevKf.size());
    const int* d_obsStart = c.in(v.mpObsStart.data(), v.mpObsStart.size());
    const int* d_obsKf = c.in(v.mpObsKf.data(), v.mpObsKf.size());
    const uint8_t* d_mpFlags = c.in(v.mpFlags.data(), v.mpFlags.size());
    std::vector<int> frame(cap, -1);
    std::copy(v.frameMp.begin(), v.frameMp.end(), frame.begin());
    int* d_frame = c.in(frame.data(), frame.size());
    const int *d_count = c.in(&count, 1), *d_last = c.in(&v.lastKf, 1);
    int *d_localKf = c.template out<int>(kfOut), *d_localMp = c.template out<int>(mpCap), *d_frameLocal = c.template out<int>(cap);
    int *d_votes = c.template out<int>(std::max(v.nkf, 1)), *d_scalars = c.template out<int>(4);   // nLocalKf, refKf, nLocalMp, overflow
    const int rc = morb_update_local_map_batch(h_, 1, v.nkf, v.kfCap, d_kfMp, d_kfCount, d_kfFlags, d_kfOrder, d_covis, v.ncovis, d_childStart,
                                               d_child, d_parent, d_prevKf, v.nmp, d_obsStart, d_obsKf, d_mpFlags, cap, d_frame, d_count, d_last,
                                               v.inertial ? 1 : 0, kfOut, d_localKf, d_scalars, d_scalars + 1, mpCap, d_localMp, d_scalars + 2,
                                               d_frameLocal, d_votes, d_scalars + 3, nullptr);
    if (rc < 0) throw std::runtime_error(morb_last_error());
    const std::vector<int> s = c.fetch(d_scalars, 4);
    if (s[3] != 0) throw std::runtime_error("Tracking::UpdateLocalMap: a list longer than its table");   // cannot happen: see kfOut / mpCap
    v.localKf = c.fetch(d_localKf, (size_t)s[0]);
    v.localMp = c.fetch(d_localMp, (size_t)s[2]);
    v.refKf = s[1];
    v.votes = c.fetch(d_votes, (size_t)v.nkf);
    frame = c.fetch(d_frame, (size_t)cap);
    std::vector<int> fl = c.fetch(d_frameLocal, (size_t)cap);
    v.frameMp.assign(frame.begin(), frame.begin() + count);
    v.frameLocal.assign(fl.begin(), fl.begin() + count);
  }

  // The map reachable from the atlas, the voting frame and the last keyframe, as tables; fills rowKF / rowMP.  No GPU call.
  void Flatten(Frame& voting, LocalMapView& v) {
    rowKF.clear(); rowMP.clear();
    std::map<KeyFrame*, int> kfRow;
    std::map<MapPoint*, int> mpRow;
    auto kf = [&](KeyFrame* p) -> int {
      if (!p) return -1;
      auto it = kfRow.find(p);
      if (it != kfRow.end()) return it->second;
      kfRow[p] = (int)rowKF.size(); rowKF.push_back(p);
      return (int)rowKF.size() - 1;
    };
    auto mp = [&](MapPoint* p) -> int {
      if (!p) return -1;
      auto it = mpRow.find(p);
      if (it != mpRow.end()) return it->second;
      mpRow[p] = (int)rowMP.size(); rowMP.push_back(p);
      return (int)rowMP.size() - 1;
    };
    for (KeyFrame* p : mpAtlas->GetAllKeyFrames()) kf(p);
    for (MapPoint* p : mpAtlas->GetAllMapPoints()) mp(p);
    v = LocalMapView();
    v.lastKf = kf(mCurrentFrame.mpLastKeyFrame);
    v.frameMp.assign(voting.N, -1);
    for (int i = 0; i < voting.N; ++i) v.frameMp[i] = mp(voting.mvpMapPoints[i]);
    // Rows grow while the graph is walked: both loops run until nothing new is reached.
    std::vector<std::vector<int>> rows, cov, kids, obs;
    std::vector<int> par, prev;
    size_t doneKF = 0, doneMP = 0;
    while (doneKF < rowKF.size() || doneMP < rowMP.size()) {
      for (; doneKF < rowKF.size(); ++doneKF) {
        KeyFrame* p = rowKF[doneKF];
        std::vector<int> r, cv, ch;
        for (MapPoint* q : p->GetMapPointMatches()) r.push_back(mp(q));
        for (KeyFrame* q : p->GetBestCovisibilityKeyFrames(10)) cv.push_back(kf(q));
        for (KeyFrame* q : p->GetChilds()) ch.push_back(kf(q));   // the set's order
        rows.push_back(r); cov.push_back(cv); kids.push_back(ch);
        par.push_back(kf(p->GetParent()));
        prev.push_back(kf(p->mPrevKF));
      }
      for (; doneMP < rowMP.size(); ++doneMP) {
        std::vector<int> o;
        for (const auto& kv : rowMP[doneMP]->GetObservations()) o.push_back(kf(kv.first));
        obs.push_back(o);
      }
    }
    v.nkf = (int)rowKF.size(); v.nmp = (int)rowMP.size();
    for (const auto& r : rows) v.kfCap = std::max(v.kfCap, (int)r.size());
    for (const auto& r : cov) v.ncovis = std::max(v.ncovis, (int)r.size());
    v.kfMp.assign((size_t)v.nkf * v.kfCap, -1); v.covis.assign((size_t)v.nkf * v.ncovis, -1);
    v.kfCount.resize(v.nkf); v.kfFlags.resize(v.nkf); v.kfOrder.resize(v.nkf); v.parent = par; v.prevKf = prev;
    v.childStart.assign(1, 0);
    std::vector<KeyFrame*> sorted(rowKF);
    std::sort(sorted.begin(), sorted.end(), std::less<KeyFrame*>());
    for (int p = 0; p < v.nkf; ++p) v.kfOrder[kfRow[sorted[p]]] = p;
    for (int k = 0; k < v.nkf; ++k) {
      std::copy(rows[k].begin(), rows[k].end(), v.kfMp.begin() + (size_t)k * v.kfCap);
      std::copy(cov[k].begin(), cov[k].end(), v.covis.begin() + (size_t)k * v.ncovis);
      v.kfCount[k] = (int)rows[k].size();
      v.kfFlags[k] = rowKF[k]->isBad() ? morblm::LM_BAD : 0;
      v.child.insert(v.child.end(), kids[k].begin(), kids[k].end());
      v.childStart.push_back((int)v.child.size());
    }
    v.mpFlags.resize(v.nmp);
    v.mpObsStart.assign(1, 0);
    for (int m = 0; m < v.nmp; ++m) {
      v.mpFlags[m] = rowMP[m]->isBad() ? morblm::LM_BAD : 0;
      v.mpObsKf.insert(v.mpObsKf.end(), obs[m].begin(), obs[m].end());
      v.mpObsStart.push_back((int)v.mpObsKf.size());
    }
    v.inertial = IsInertial(mSensor);
  }

  void UpdateLocalMap() {
    // This is for visualization
    mpAtlas->SetReferenceMapPoints(mvpLocalMapPoints);
    // Each map point vote for the keyframes in which it has been observed: the current frame's, or the last frame's (:3223-3224)
    Frame& voting = (!mpAtlas->isImuInitialized() || (mCurrentFrame.mnId < mnLastRelocFrameId + 2)) ? mCurrentFrame : mLastFrame;
    LocalMapView v;
    Flatten(voting, v);
    UpdateLocalMap(v);
    for (int i = 0; i < voting.N; ++i)
      if (v.frameMp[i] < 0) voting.mvpMapPoints[i] = static_cast<MapPoint*>(NULL);   // the bad ones (:3237 / :3257); the others were NULL already
    mvpLocalKeyFrames.clear();
    for (int r : v.localKf) {
      mvpLocalKeyFrames.push_back(rowKF[r]);
      rowKF[r]->mnTrackReferenceForFrame = mCurrentFrame.mnId;
    }
    mvpLocalMapPoints.clear();
    for (int r : v.localMp) {
      mvpLocalMapPoints.push_back(rowMP[r]);
      rowMP[r]->mnTrackReferenceForFrame = mCurrentFrame.mnId;
    }
    if (v.refKf >= 0) {
      mpReferenceKF = rowKF[v.refKf];
      mCurrentFrame.mpReferenceKF = mpReferenceKF;
    }
  }

 private:
  int device_;
  morb_matcher* h_ = nullptr;
};

}  // namespace ORB_SLAM3
