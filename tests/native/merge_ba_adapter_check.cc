// Optimizer::LocalBundleAdjustment(MergeBAView&, bool*) of include/morb/Optimizer.h on one problem read from a file, and the reference-typed
// LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag) on a mock map (tests/native/mock_merge_ba) built from the same problem.
// Run as `merge_ba_adapter_check <in.bin> <out.bin>`; tests/test_merge_ba_adapter_gpu.py compares what it dumps with the C entry.
// in.bin: int nKF, nMP, nE, kb8; float cam8[8] (pinhole: fx fy cx cy bf); float kfPose[nKF][7]; uint8 kfFixed[nKF]; float mpPos[nMP][3];
// int eKF[nE], eMP[nE]; float eObs[nE][3], eInvSigma2[nE].
// out.bin: the view call's kfPose, mpPos, eraseFlag, levelFlag, stats[6]; then the mock map after the member: per keyframe pose (7 floats), per
// keyframe SetPose calls (int), per point position (3 floats), per point UpdateNormalAndDepth calls (int), per edge erased (uint8), per keyframe
// and per point the merge mark (int).
#include <cstdio>
#include <fstream>
#include <vector>

#include "merge_ba_mock.h"
#include "Optimizer.h"

using namespace ORB_SLAM3;
std::mutex ORB_SLAM3::MapPoint::mGlobalMutex;

template <class T> static void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), n * sizeof(T)); }
template <class T> static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), n * sizeof(T)); }

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: %s in.bin out.bin\n", argv[0]); return 2; }
  std::ifstream in(argv[1], std::ios::binary);
  int hd[4];
  rd(in, hd, 4);
  const int nKF = hd[0], nMP = hd[1], nE = hd[2];
  const bool kb8 = hd[3] != 0;
  float cam[8];
  rd(in, cam, 8);
  std::vector<float> kfPose((size_t)nKF * 7), mpPos((size_t)nMP * 3), eObs((size_t)nE * 3), eInv(nE);
  std::vector<uint8_t> kfFixed(nKF);
  std::vector<int> eKF(nE), eMP(nE);
  rd(in, kfPose.data(), kfPose.size()); rd(in, kfFixed.data(), nKF); rd(in, mpPos.data(), mpPos.size());
  rd(in, eKF.data(), nE); rd(in, eMP.data(), nE); rd(in, eObs.data(), eObs.size()); rd(in, eInv.data(), nE);
  if (!in) { std::printf("short input\n"); return 2; }
  std::ofstream out(argv[2], std::ios::binary);
  bool bStop = false;
  {   // (1) the view-taking form
    std::vector<float> pose = kfPose, pos = mpPos;
    MergeBAView g;
    g.nKF = nKF; g.nMP = nMP; g.nE = nE; g.kfPose = pose.data(); g.kfFixed = kfFixed.data(); g.mpPos = pos.data(); g.eKF = eKF.data(); g.eMP = eMP.data();
    g.eObs = eObs.data(); g.eInvSigma2 = eInv.data();
    if (kb8) g.camL8 = cam; else { g.fx = cam[0]; g.fy = cam[1]; g.cx = cam[2]; g.cy = cam[3]; g.mbf = cam[4]; }
    Optimizer::LocalBundleAdjustment(g, &bStop);
    wr(out, pose.data(), pose.size()); wr(out, pos.data(), pos.size()); wr(out, g.eraseFlag.data(), nE); wr(out, g.levelFlag.data(), nE); wr(out, g.stats, 6);
  }
  {   // (2) the reference signature on a mock map: keypoint i of a keyframe is its i-th edge
    MBMap map;
    GeometricCamera camera;
    camera.mvParameters.assign(cam, cam + (kb8 ? 8 : 4));
    std::vector<MBKeyFrame> kfs(nKF);
    std::vector<MBMapPoint> mps(nMP);
    for (int j = 0; j < nMP; ++j) { mps[j].mnId = j; mps[j].mpMap = &map; mps[j].mWorldPos = Eigen::Vector3f(mpPos[3 * j], mpPos[3 * j + 1], mpPos[3 * j + 2]); }
    for (int k = 0; k < nKF; ++k) {
      MBKeyFrame& K = kfs[k];
      K.mnId = 1 + k; K.mpMap = &map; K.mpCamera = &camera;
      if (!kb8) { K.fx = cam[0]; K.fy = cam[1]; K.cx = cam[2]; K.cy = cam[3]; K.mbf = cam[4]; }
      for (int c = 0; c < 4; ++c) K.mTcw.q[c] = kfPose[7 * k + c];
      for (int c = 0; c < 3; ++c) K.mTcw.t[c] = kfPose[7 * k + 4 + c];
    }
    std::vector<int> slot(nE);
    for (int e = 0; e < nE; ++e) {
      MBKeyFrame& K = kfs[eKF[e]];
      slot[e] = (int)K.mvKeysUn.size();
      cv::KeyPoint kp;
      kp.pt.x = eObs[3 * e]; kp.pt.y = eObs[3 * e + 1]; kp.octave = slot[e];
      K.mvKeysUn.push_back(kp); K.mvuRight.push_back(kb8 ? -1.f : eObs[3 * e + 2]); K.mvInvLevelSigma2.push_back(eInv[e]);
      K.mvpMapPoints.push_back(&mps[eMP[e]]);
      K.N = (int)K.mvKeysUn.size();
      mps[eMP[e]].AddObservation(&K, slot[e], -1);
    }
    std::vector<MBKeyFrame*> vpLocalCurrentWindowKFs, vpMergeConnectedKFs;
    for (int k = 0; k < nKF; ++k) (kfFixed[k] ? vpMergeConnectedKFs : vpLocalCurrentWindowKFs).push_back(&kfs[k]);
    MBKeyFrame* mpCurrentKF = vpLocalCurrentWindowKFs.front();
    Optimizer::LocalBundleAdjustment(mpCurrentKF, vpLocalCurrentWindowKFs, vpMergeConnectedKFs, &bStop);
    for (int k = 0; k < nKF; ++k) { wr(out, kfs[k].mTcw.q, 4); wr(out, kfs[k].mTcw.t, 3); }
    for (int k = 0; k < nKF; ++k) wr(out, &kfs[k].nSetPose, 1);
    for (int j = 0; j < nMP; ++j) wr(out, mps[j].mWorldPos.v, 3);
    for (int j = 0; j < nMP; ++j) wr(out, &mps[j].nUpdates, 1);
    for (int e = 0; e < nE; ++e) { const uint8_t gone = kfs[eKF[e]].mvpMapPoints[slot[e]] == nullptr ? 1 : 0; wr(out, &gone, 1); }
    for (int k = 0; k < nKF; ++k) { const int m = (int)kfs[k].mnBALocalForMerge; wr(out, &m, 1); }
    for (int j = 0; j < nMP; ++j) { const int m = (int)mps[j].mnBALocalForMerge; wr(out, &m, 1); }
  }
  return out ? 0 : 1;
}
