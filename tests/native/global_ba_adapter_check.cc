// Optimizer::BundleAdjustment(GlobalBAView&, int, bool, bool*) of include/morb/Optimizer.h on one problem read from a file, and the
// reference-typed WholeMapBundleAdjustment on a mock map (tests/native/mock_global_ba) built from the same problem, once with nLoopKF the
// origin keyframe's id and once with another; built with MORB_WHOLE_MAP_BUNDLE_ADJUSTMENT defined, the second run goes through
// GlobalBundleAdjustemnt with LoopClosing.cc:2302's arguments.  Run as `global_ba_adapter_check <in.bin> <out.bin>`;
// tests/test_global_ba_adapter_gpu.py compares what it dumps with the C entry.
// in.bin: int nKF, nMP, nE, kb8; float camL[8] (pinhole: fx fy cx cy bf), camR[8], Trl7[7] (identity rotation); float kfPose[nKF][7]; uint8
// kfFixed[nKF] (keyframe 0 alone); float mpPos[nMP][3]; int eKF[nE], eMP[nE]; float eObs[nE][3]; uint8 eRight[nE]; float eInvSigma2[nE].
// out.bin: the view call's kfPose, mpPos, stats[4], chi2[2]; the mock map after the first run: per keyframe pose (7 floats) and SetPose calls
// (int), per point position (3 floats) and UpdateNormalAndDepth calls (int); after the second: per keyframe mTcwGBA (7 floats) and
// mnBAGlobalForKF (int), per point mPosGBA (3 floats) and mnBAGlobalForKF (int).
#define MORB_WHOLE_MAP_BUNDLE_ADJUSTMENT
#include <cstdio>
#include <fstream>
#include <vector>

#include "global_ba_mock.h"
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
  float camL[8], camR[8], trl7[7];
  rd(in, camL, 8); rd(in, camR, 8); rd(in, trl7, 7);
  std::vector<float> kfPose((size_t)nKF * 7), mpPos((size_t)nMP * 3), eObs((size_t)nE * 3), eInv(nE);
  std::vector<uint8_t> kfFixed(nKF), eRight(nE);
  std::vector<int> eKF(nE), eMP(nE);
  rd(in, kfPose.data(), kfPose.size()); rd(in, kfFixed.data(), nKF); rd(in, mpPos.data(), mpPos.size());
  rd(in, eKF.data(), nE); rd(in, eMP.data(), nE); rd(in, eObs.data(), eObs.size()); rd(in, eRight.data(), nE); rd(in, eInv.data(), nE);
  if (!in) { std::printf("short input\n"); return 2; }
  std::ofstream out(argv[2], std::ios::binary);
  bool mbStopGBA = false;
  {   // (1) the view-taking form
    std::vector<float> pose = kfPose, pos = mpPos;
    float rig28[28] = {0};
    GlobalBAView g;
    g.nKF = nKF; g.nMP = nMP; g.nE = nE; g.kfPose = pose.data(); g.kfFixed = kfFixed.data(); g.mpPos = pos.data(); g.eKF = eKF.data(); g.eMP = eMP.data();
    g.eObs = eObs.data(); g.eInvSigma2 = eInv.data();
    if (kb8) {
      for (int k = 0; k < 8; ++k) { rig28[k] = camL[k]; rig28[8 + k] = camR[k]; }
      rig28[16] = rig28[20] = rig28[24] = 1.f;
      for (int k = 0; k < 3; ++k) rig28[25 + k] = trl7[4 + k];
      g.rig28 = rig28; g.eRight = eRight.data();
    } else { g.fx = camL[0]; g.fy = camL[1]; g.cx = camL[2]; g.cy = camL[3]; g.mbf = camL[4]; }
    Optimizer::BundleAdjustment(g, 10, false, &mbStopGBA);
    wr(out, pose.data(), pose.size()); wr(out, pos.data(), pos.size()); wr(out, g.stats, 4); wr(out, g.chi2, 2);
  }
  for (int run = 0; run < 2; ++run) {   // (2), (3) the reference signatures on a mock map: keypoint i of a keyframe is its i-th edge of that camera
    GBMap map;
    GeometricCamera cameraL, cameraR;
    cameraL.mvParameters.assign(camL, camL + (kb8 ? 8 : 4));
    cameraR.mvParameters.assign(camR, camR + 8);
    std::vector<GBKeyFrame> kfs(nKF);
    std::vector<GBMapPoint> mps(nMP);
    for (int j = 0; j < nMP; ++j) {
      mps[j].mnId = j; mps[j].mpMap = &map; mps[j].mWorldPos = Eigen::Vector3f(mpPos[3 * j], mpPos[3 * j + 1], mpPos[3 * j + 2]);
      map.points.push_back(&mps[j]);
    }
    for (int k = 0; k < nKF; ++k) {
      GBKeyFrame& K = kfs[k];
      K.mnId = 1 + k; K.mpMap = &map; K.mpCamera = &cameraL;
      if (kb8) { K.mpCamera2 = &cameraR; K.NLeft = 0; for (int c = 0; c < 3; ++c) K.mTrl.t[c] = trl7[4 + c]; }
      else { K.fx = camL[0]; K.fy = camL[1]; K.cx = camL[2]; K.cy = camL[3]; K.mbf = camL[4]; }
      for (int c = 0; c < 4; ++c) K.mTcw.q[c] = kfPose[7 * k + c];
      for (int c = 0; c < 3; ++c) K.mTcw.t[c] = kfPose[7 * k + 4 + c];
      map.keyframes.push_back(&K);
    }
    map.initKF = 1; map.origin = &kfs[0];
    for (int e = 0; e < nE; ++e) {
      GBKeyFrame& K = kfs[eKF[e]];
      GBMapPoint& P = mps[eMP[e]];
      cv::KeyPoint kp;
      kp.pt.x = eObs[3 * e]; kp.pt.y = eObs[3 * e + 1]; kp.octave = (int)K.mvInvLevelSigma2.size();
      K.mvInvLevelSigma2.push_back(eInv[e]);
      int left = -1, right = -1;
      const auto it = P.mObservations.find(&K);
      if (it != P.mObservations.end()) { left = std::get<0>(it->second); right = std::get<1>(it->second); }
      if (eRight[e]) { right = (int)K.mvKeysRight.size(); K.mvKeysRight.push_back(kp); }
      else { left = (int)K.mvKeysUn.size(); K.mvKeysUn.push_back(kp); K.mvuRight.push_back(kb8 ? -1.f : eObs[3 * e + 2]); K.N = (int)K.mvKeysUn.size(); }
      P.AddObservation(&K, left, right);
    }
    if (run == 0) {
      Optimizer::WholeMapBundleAdjustment(map.keyframes, map.points, 10, &mbStopGBA, 1, false);
      for (int k = 0; k < nKF; ++k) { wr(out, kfs[k].mTcw.q, 4); wr(out, kfs[k].mTcw.t, 3); wr(out, &kfs[k].nSetPose, 1); }
      for (int j = 0; j < nMP; ++j) { wr(out, mps[j].mWorldPos.v, 3); wr(out, &mps[j].nUpdates, 1); }
    } else {
      GBMap* pActiveMap = &map;
      const unsigned long nLoopKF = 5;
      Optimizer::GlobalBundleAdjustemnt(pActiveMap, 10, &mbStopGBA, nLoopKF, false);   // LoopClosing.cc:2302
      for (int k = 0; k < nKF; ++k) { const int m = (int)kfs[k].mnBAGlobalForKF + 100 * kfs[k].nSetPose; wr(out, kfs[k].mTcwGBA.q, 4); wr(out, kfs[k].mTcwGBA.t, 3); wr(out, &m, 1); }
      for (int j = 0; j < nMP; ++j) { const int m = (int)mps[j].mnBAGlobalForKF + 100 * mps[j].nUpdates; wr(out, mps[j].mPosGBA.v, 3); wr(out, &m, 1); }
    }
  }
  return out ? 0 : 1;
}
