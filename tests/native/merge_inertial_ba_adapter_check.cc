// Optimizer::MergeInertialBA(MergeInertialBAView&, bool*) of include/morb/Optimizer.h on one problem read from a file, and the reference-typed
// MergeInertialBA(pCurrKF, pMergeKF, pbStopFlag, pMap, corrPoses) on a mock map (tests/native/mock_merge_inertial_ba) built from the same problem.
// Run as `merge_inertial_ba_adapter_check <in.bin> <out.bin>`; tests/test_merge_inertial_ba_adapter_gpu.py compares what it dumps with the C
// entry called from Python.
// in.bin: int nKF, nMP, nE, nI, rig, nA, nB (keyframes [0, nA) are the current chain, [nA, nA + nB) the merge chain, in temporal order);
// float cam5[5] (fx fy cx cy bf), rig28[28], Tbc12[12]; float kfState[nKF][21]; uint8 kfKind[nKF];
// float mpPos[nMP][3]; int eKF[nE], eMP[nE]; float eObs[nE][3], eInvSigma2[nE]; int iKF1[nI], iKF2[nI]; morb_imu_preintegrated iPre[nI].
// out.bin: kfState, mpPos, eraseFlag, {outer iterations, LM trials, ran}; then the same after a call with the stop flag set; then the mock
// map after the member: per keyframe {readOrder, SetPose calls, SetVelocity calls, SetNewBias calls, in corrPoses} (5 ints), the pose it holds
// (R 9, t 3 floats), velocity (3), bias as gyro, acc (6), corrPoses' quaternion xyzw, translation and scale (8 doubles); per point {readOrder,
// UpdateNormalAndDepth calls} (2 ints) and position (3 floats); per edge erased (uint8); per link SetNewBias calls on its preintegration (int);
// the map's change index (int).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "merge_inertial_ba_mock.h"
#include "Optimizer.h"

using namespace ORB_SLAM3;

template <class T> static void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), n * sizeof(T)); }
template <class T> static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), n * sizeof(T)); }

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: %s in.bin out.bin\n", argv[0]); return 2; }
  std::ifstream in(argv[1], std::ios::binary);
  int hd[7];
  rd(in, hd, 7);
  const int nKF = hd[0], nMP = hd[1], nE = hd[2], nI = hd[3];
  const bool rig = hd[4] != 0;
  const int nA = hd[5], nB = hd[6];
  float cam[5], rig28[28], Tbc[12];
  rd(in, cam, 5); rd(in, rig28, 28); rd(in, Tbc, 12);
  std::vector<float> kfState((size_t)nKF * 21), mpPos((size_t)nMP * 3), eObs((size_t)nE * 3), eInv(nE);
  std::vector<uint8_t> kfKind(nKF);
  std::vector<int> eKF(nE), eMP(nE), iKF1(nI), iKF2(nI);
  std::vector<morb_imu_preintegrated> iPre(nI);
  rd(in, kfState.data(), kfState.size()); rd(in, kfKind.data(), nKF); rd(in, mpPos.data(), mpPos.size());
  rd(in, eKF.data(), nE); rd(in, eMP.data(), nE); rd(in, eObs.data(), eObs.size()); rd(in, eInv.data(), nE);
  rd(in, iKF1.data(), nI); rd(in, iKF2.data(), nI); rd(in, iPre.data(), nI);
  if (!in) { std::printf("short input\n"); return 2; }
  std::ofstream out(argv[2], std::ios::binary);
  for (bool bStop : {false, true}) {
    std::vector<float> state = kfState, pos = mpPos;
    MergeInertialBAView g;
    g.nKF = nKF; g.nMP = nMP; g.nE = nE; g.nI = nI; g.kfState = state.data(); g.kfKind = kfKind.data(); g.mpPos = pos.data();
    g.eKF = eKF.data(); g.eMP = eMP.data(); g.eObs = eObs.data(); g.eInvSigma2 = eInv.data(); g.iKF1 = iKF1.data(); g.iKF2 = iKF2.data(); g.iPre = iPre.data();
    g.fx = cam[0]; g.fy = cam[1]; g.cx = cam[2]; g.cy = cam[3]; g.mbf = cam[4];
    if (rig) g.rig28 = rig28;
    std::memcpy(g.Tbc12, Tbc, sizeof Tbc);
    bool flag = bStop;
    Optimizer::MergeInertialBA(g, &flag);
    const int stats[3] = {g.outerIterations, g.lmTrials, g.ran ? 1 : 0};
    wr(out, state.data(), state.size()); wr(out, pos.data(), pos.size()); wr(out, g.eraseFlag.data(), nE); wr(out, stats, 3);
  }
  {   // the reference signature on a mock map: keypoint i of a keyframe is its i-th edge
    MIMap map;
    GeometricCamera camL, camR;
    if (rig) { camL.mvParameters.assign(rig28, rig28 + 8); camR.mvParameters.assign(rig28 + 8, rig28 + 16); }
    std::vector<MIKeyFrame> kfs(nKF);
    std::vector<MIMapPoint> mps(nMP);
    std::vector<MIPreintegrated> pre(nI);
    for (int j = 0; j < nMP; ++j) { mps[j].mnId = j; mps[j].mWorldPos = Eigen::Vector3f(mpPos[3 * j], mpPos[3 * j + 1], mpPos[3 * j + 2]); }
    for (int k = 0; k < nKF; ++k) {
      MIKeyFrame& K = kfs[k];
      K.mnId = k < nA ? 1000 + k : 1 + k;   // the current keyframe (the last of its chain) is the newest of all
      K.fx = cam[0]; K.fy = cam[1]; K.cx = cam[2]; K.cy = cam[3]; K.mbf = cam[4];
      if (rig) { K.mpCamera = &camL; K.mpCamera2 = &camR; for (int c = 0; c < 9; ++c) K.mTrl.R[c] = rig28[16 + c]; for (int c = 0; c < 3; ++c) K.mTrl.t[c] = rig28[25 + c]; }
      for (int c = 0; c < 9; ++c) K.mImuCalib.mTbc.R[c] = Tbc[c];
      for (int c = 0; c < 3; ++c) K.mImuCalib.mTbc.t[c] = Tbc[9 + c];
      const float* s = &kfState[(size_t)21 * k];
      for (int c = 0; c < 9; ++c) K.mRwb.m[c] = s[c];
      for (int c = 0; c < 3; ++c) { K.mOwb(c) = s[9 + c]; K.mVw(c) = s[12 + c]; }
      K.mImuBias = IMU::Bias(s[18], s[19], s[20], s[15], s[16], s[17]);
      K.bImu = kfKind[k] != 2;
      if ((k > 0 && k < nA) || (k > nA && k < nA + nB)) { K.mPrevKF = &kfs[k - 1]; kfs[k - 1].mNextKF = &K; }
    }
    for (int e = 0; e < nE; ++e) {
      MIKeyFrame& K = kfs[eKF[e]];
      const int idx = (int)K.mvKeysUn.size();
      cv::KeyPoint kp; kp.pt.x = eObs[3 * e]; kp.pt.y = eObs[3 * e + 1]; kp.octave = idx;
      K.mvKeysUn.push_back(kp); K.mvuRight.push_back(eObs[3 * e + 2]); K.mvInvLevelSigma2.push_back(eInv[e]); K.mvpMapPoints.push_back(&mps[eMP[e]]);
      mps[eMP[e]].mObservations[&K] = std::make_tuple(idx, -1);
    }
    for (int i = 0; i < nI; ++i) {
      const morb_imu_preintegrated& r = iPre[i];
      MIPreintegrated& P = pre[i];
      P.dT = r.dT;
      auto m3 = [](Eigen::Matrix3f& M, const float* v) { for (int c = 0; c < 9; ++c) M.m[c] = v[c]; };
      auto v3 = [](Eigen::Vector3f& V, const float* v) { for (int c = 0; c < 3; ++c) V.v[c] = v[c]; };
      m3(P.dR, r.dR); v3(P.dV, r.dV); v3(P.dP, r.dP); m3(P.JRg, r.JRg); m3(P.JVg, r.JVg); m3(P.JVa, r.JVa); m3(P.JPg, r.JPg); m3(P.JPa, r.JPa);
      for (int c = 0; c < 225; ++c) P.C.m[c] = r.C[c];
      P.b = IMU::Bias(r.b[0], r.b[1], r.b[2], r.b[3], r.b[4], r.b[5]);
      for (int c = 0; c < 6; ++c) { P.Nga.d.v[c] = r.nga[c]; P.NgaWalk.d.v[c] = r.ngaWalk[c]; }
      v3(P.avgA, r.avgA); v3(P.avgW, r.avgW);
      kfs[iKF2[i]].mpImuPreintegrated = &P;
    }
    MIKeyFrame *mpCurrentKF = &kfs[nA - 1], *mpMergeMatchedKF = &kfs[nA + (nB - 1 < 3 ? nB - 1 : 3)];
    MIMap* pCurrentMap = &map;
    std::map<MIKeyFrame*, g2o::Sim3> vCorrectedSim3;
    bool bStop = false;
    Optimizer::MergeInertialBA(mpCurrentKF, mpMergeMatchedKF, &bStop,
                               pCurrentMap, vCorrectedSim3);
    for (int k = 0; k < nKF; ++k) {
      MIKeyFrame& K = kfs[k];
      const bool in = vCorrectedSim3.count(&K) != 0;
      const int counts[5] = {K.readOrder, K.nSetPose, K.nSetVelocity, K.nSetNewBias, in ? 1 : 0};
      wr(out, counts, 5); wr(out, K.mTcw.R, 9); wr(out, K.mTcw.t, 3); wr(out, K.mVw.v, 3);
      const float bias[6] = {K.mImuBias.bwx, K.mImuBias.bwy, K.mImuBias.bwz, K.mImuBias.bax, K.mImuBias.bay, K.mImuBias.baz};
      wr(out, bias, 6);
      double S[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (in) { const g2o::Sim3& c = vCorrectedSim3[&K]; S[0] = c.rotation().x(); S[1] = c.rotation().y(); S[2] = c.rotation().z(); S[3] = c.rotation().w();
                for (int q = 0; q < 3; ++q) S[4 + q] = c.translation()(q); S[7] = c.scale(); }
      wr(out, S, 8);
    }
    for (int j = 0; j < nMP; ++j) { const int c[2] = {mps[j].readOrder, mps[j].nUpdates}; wr(out, c, 2); wr(out, mps[j].mWorldPos.v, 3); }
    std::vector<uint8_t> gone(nE);
    { std::vector<int> next(nKF, 0); for (int e = 0; e < nE; ++e) gone[e] = kfs[eKF[e]].mvpMapPoints[next[eKF[e]]++] == nullptr ? 1 : 0; }
    wr(out, gone.data(), nE);
    for (int i = 0; i < nI; ++i) wr(out, &pre[i].nSetNewBias, 1);
    wr(out, &map.changes, 1);
  }
  std::printf("merge inertial ba adapter ok\n");
  return 0;
}
