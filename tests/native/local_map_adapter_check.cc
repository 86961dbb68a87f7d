// include/morb/Tracking.h against the mocks of tests/native/mock_tracking.
//   local_map_adapter_check flatten      a hand-made map through TrackingT::Flatten, no GPU call: rows, d_kfOrder, tables -> "flatten ok"
//   local_map_adapter_check IN OUT       the map of file IN (written by tests/test_local_map_adapter_gpu.py) through the member
//                                        UpdateLocalMap() on the GPU; OUT takes what the member wrote back.
// The keyframe objects of the second mode live in one array, keyframe `row` at slot order[row]: the pointer order is the file's.
// IN:  nkf nmp sensor imuInitialized frameId lastRelocFrameId lastKf
//      per keyframe: order bad parent prev  ncovis covis..  nrow row..
//      per point:    bad nobs keyframe..
//      current frame: N entry..      last frame: N entry..
// OUT: K n row..   R row   P n row..   C N entry.. (current frame)   L N entry.. (last frame)   SK n row.. (stamped keyframes)   SP n row..
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>

#include "tracking_mock.h"

#include "Tracking.h"

using namespace ORB_SLAM3;
typedef TrackingT<Frame, KeyFrame, MapPoint, Atlas> Tracker;

static int flatten_check() {
  // three keyframes placed so that the pointer order is 2 < 0 < 1; keyframe 1 is not in the atlas and is reached as 0's parent
  std::vector<KeyFrame> pool(3);
  KeyFrame *k2 = &pool[0], *k0 = &pool[1], *k1 = &pool[2];
  std::vector<MapPoint> pts(4);
  k0->mvpMapPoints = {&pts[0], nullptr, &pts[1]};
  k2->mvpMapPoints = {&pts[1], &pts[3]};       // pts[3] is not in the atlas either
  k0->mpParent = k1; k1->mspChildrens = {k0, k2}; k2->mpParent = k1;
  k0->mvpOrdered = {k2}; k2->mPrevKF = k0; k1->mbBad = true; pts[1].mbBad = true;
  pts[0].mObservations[k0] = std::make_tuple(0, -1);
  pts[1].mObservations[k0] = std::make_tuple(2, -1); pts[1].mObservations[k2] = std::make_tuple(0, -1);
  pts[3].mObservations[k2] = std::make_tuple(1, -1);
  Atlas atlas;
  atlas.mvpKeyFrames = {k0, k2};
  atlas.mvpMapPoints = {&pts[0], &pts[1], &pts[2]};
  Tracker T;
  T.mpAtlas = &atlas; T.mSensor = 4;
  T.mCurrentFrame.N = 3; T.mCurrentFrame.mvpMapPoints = {&pts[1], nullptr, &pts[0]}; T.mCurrentFrame.mpLastKeyFrame = k2;
  LocalMapView v;
  T.Flatten(T.mCurrentFrame, v);
  bool ok = v.nkf == 3 && v.nmp == 4 && T.rowKF == std::vector<KeyFrame*>({k0, k2, k1}) && T.rowMP[3] == &pts[3];
  ok = ok && v.kfOrder == std::vector<int>({1, 0, 2}) && v.kfCap == 3 && v.ncovis == 1 && v.inertial && v.lastKf == 1;
  ok = ok && v.kfMp == std::vector<int>({0, -1, 1, 1, 3, -1, -1, -1, -1}) && v.kfCount == std::vector<int>({3, 2, 0});
  ok = ok && v.covis == std::vector<int>({1, -1, -1}) && v.parent == std::vector<int>({2, 2, -1}) && v.prevKf == std::vector<int>({-1, 0, -1});
  ok = ok && v.childStart == std::vector<int>({0, 0, 0, 2}) && v.child == std::vector<int>({1, 0});   // the set's order: k2 before k0
  ok = ok && v.kfFlags == std::vector<uint8_t>({0, 0, 1}) && v.mpFlags == std::vector<uint8_t>({0, 1, 0, 0});
  ok = ok && v.mpObsStart == std::vector<int>({0, 1, 3, 3, 4}) && v.mpObsKf == std::vector<int>({0, 1, 0, 1}) && v.frameMp == std::vector<int>({1, -1, 0});
  std::printf(ok ? "flatten ok\n" : "flatten MISMATCH\n");
  return ok ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "flatten")) return flatten_check();
  if (argc != 3) return 2;
  std::ifstream in(argv[1]);
  int nkf, nmp, sensor, imuInit, lastKf;
  long frameId, lastReloc;
  in >> nkf >> nmp >> sensor >> imuInit >> frameId >> lastReloc >> lastKf;
  std::vector<KeyFrame> pool(nkf);
  std::vector<MapPoint> pts(nmp);
  std::vector<KeyFrame*> at(nkf);
  std::vector<std::vector<int>> covis(nkf), rows(nkf);
  std::vector<int> parent(nkf), prev(nkf);
  for (int k = 0; k < nkf; ++k) {
    int order, bad, n;
    in >> order >> bad >> parent[k] >> prev[k];
    at[k] = &pool[order];
    at[k]->mbBad = bad != 0;
    in >> n; covis[k].resize(n); for (int& c : covis[k]) in >> c;
    in >> n; rows[k].resize(n); for (int& r : rows[k]) in >> r;
  }
  for (int k = 0; k < nkf; ++k) {
    for (int c : covis[k]) at[k]->mvpOrdered.push_back(at[c]);
    for (int r : rows[k]) at[k]->mvpMapPoints.push_back(r < 0 ? nullptr : &pts[r]);
    if (parent[k] >= 0) { at[k]->mpParent = at[parent[k]]; at[parent[k]]->mspChildrens.insert(at[k]); }
    if (prev[k] >= 0) at[k]->mPrevKF = at[prev[k]];
  }
  for (int m = 0; m < nmp; ++m) {
    int bad, n;
    in >> bad >> n;
    pts[m].mbBad = bad != 0;
    for (int j = 0; j < n; ++j) { int k; in >> k; pts[m].mObservations[at[k]] = std::make_tuple(j, -1); }
  }
  Atlas atlas;
  atlas.mbImuInitialized = imuInit != 0;
  for (int k = 0; k < nkf; ++k) atlas.mvpKeyFrames.push_back(at[k]);
  for (int m = 0; m < nmp; ++m) atlas.mvpMapPoints.push_back(&pts[m]);
  Tracker T;
  T.mpAtlas = &atlas; T.mSensor = sensor; T.mnLastRelocFrameId = (unsigned int)lastReloc;
  for (Frame* f : {&T.mCurrentFrame, &T.mLastFrame}) {
    in >> f->N;
    for (int i = 0; i < f->N; ++i) { int r; in >> r; f->mvpMapPoints.push_back(r < 0 ? nullptr : &pts[r]); }
  }
  T.mCurrentFrame.mnId = (unsigned long)frameId; T.mLastFrame.mnId = (unsigned long)frameId - 1;
  T.mCurrentFrame.mpLastKeyFrame = lastKf >= 0 ? at[lastKf] : nullptr;
  if (!in) { std::fprintf(stderr, "bad input\n"); return 2; }
  T.mvpLocalMapPoints = {&pts[0]};   // what the visualisation hand-over sees
  try {
    T.UpdateLocalMap();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  if (atlas.mvpReferenceMapPoints != std::vector<MapPoint*>({&pts[0]})) return 3;
  auto kfRow = [&](KeyFrame* p) { return p ? (int)(p - pool.data()) : -1; };   // slot, mapped back below
  std::vector<int> rowOfSlot(nkf);
  for (int k = 0; k < nkf; ++k) rowOfSlot[kfRow(at[k])] = k;
  std::ofstream out(argv[2]);
  out << "K " << T.mvpLocalKeyFrames.size();
  for (KeyFrame* p : T.mvpLocalKeyFrames) out << ' ' << rowOfSlot[kfRow(p)];
  const bool same = T.mpReferenceKF == T.mCurrentFrame.mpReferenceKF;
  out << "\nR " << (T.mpReferenceKF && same ? rowOfSlot[kfRow(T.mpReferenceKF)] : (same ? -1 : -2));
  out << "\nP " << T.mvpLocalMapPoints.size();
  for (MapPoint* p : T.mvpLocalMapPoints) out << ' ' << (int)(p - pts.data());
  const char* tag[2] = {"C", "L"};
  int t = 0;
  for (Frame* f : {&T.mCurrentFrame, &T.mLastFrame}) {
    out << "\n" << tag[t++] << ' ' << f->N;
    for (MapPoint* p : f->mvpMapPoints) out << ' ' << (p ? (int)(p - pts.data()) : -1);
  }
  std::vector<int> sk, sp;
  for (int k = 0; k < nkf; ++k) if (at[k]->mnTrackReferenceForFrame == (unsigned long)frameId) sk.push_back(k);
  for (int m = 0; m < nmp; ++m) if (pts[m].mnTrackReferenceForFrame == (unsigned long)frameId) sp.push_back(m);
  out << "\nSK " << sk.size(); for (int k : sk) out << ' ' << k;
  out << "\nSP " << sp.size(); for (int m : sp) out << ' ' << m;
  out << "\n";
  return 0;
}
