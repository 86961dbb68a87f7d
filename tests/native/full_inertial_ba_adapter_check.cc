// Optimizer::FullInertialBA(FullInertialBAView&, its, bInit, priorG, priorA, pbStopFlag, role) of include/morb/Optimizer.h on one problem read
// from a file, and the reference-typed FullInertialBA(pMap, its, bFixLocal, nLoopId, pbStopFlag, bInit, priorG, priorA) on a mock map
// (tests/native/mock_full_inertial_ba) built from the same problem, once with nLoopId == 0 and no stop flag (LocalMapping's form) and once with
// a loop id and a stop flag (LoopClosing's).  Run as `full_inertial_ba_adapter_check <in.bin> <out.bin>`;
// tests/test_full_inertial_ba_adapter_gpu.py compares what it dumps with the C entry called from Python.
// in.bin: int nKF, nMP, nE, nI, rig, its, bInit; float cam5[5] (fx fy cx cy bf), rig28[28], Tbc12[12], priors[2], bias6[6] (the last keyframe's);
// float kfState[nKF][21]; uint8 kfKind[nKF] (0 and 3 only: a kind-3 keyframe has no IMU); float mpPos[nMP][3]; int eKF[nE], eMP[nE]; float
// eObs[nE][3]; uint8 eRight[nE]; float eInvSigma2[nE]; int iKF1[nI], iKF2[nI]; morb_imu_preintegrated iPre[nI].
// out.bin: the view call's kfState, mpPos, bias6, stats[4], chi2[2]; then per run of the member, per keyframe {SetPose calls, SetVelocity calls,
// SetNewBias calls, mnBAGlobalForKF} (4 ints), pose R 9 and t 3, velocity 3, bias as gyro, acc 6 (the keyframe's own members in the first run,
// the GBA members in the second); per point {UpdateNormalAndDepth calls, mnBAGlobalForKF} (2 ints) and position 3; per link SetNewBias calls on
// its preintegration (int); the map's change index (int).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "full_inertial_ba_mock.h"
#include "Optimizer.h"

using namespace ORB_SLAM3;

template <class T> static void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), n * sizeof(T)); }
template <class T> static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), n * sizeof(T)); }

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: %s in.bin out.bin\n", argv[0]); return 2; }
  std::ifstream in(argv[1], std::ios::binary);
  int hd[7];
  rd(in, hd, 7);
  const int nKF = hd[0], nMP = hd[1], nE = hd[2], nI = hd[3], its = hd[5];
  const bool rig = hd[4] != 0, bInit = hd[6] != 0;
  float cam[5], rig28[28], Tbc[12], priors[2], bias6[6];
  rd(in, cam, 5); rd(in, rig28, 28); rd(in, Tbc, 12); rd(in, priors, 2); rd(in, bias6, 6);
  std::vector<float> kfState((size_t)nKF * 21), mpPos((size_t)nMP * 3), eObs((size_t)nE * 3), eInv(nE);
  std::vector<uint8_t> kfKind(nKF), eRight(nE);
  std::vector<int> eKF(nE), eMP(nE), iKF1(nI), iKF2(nI);
  std::vector<morb_imu_preintegrated> iPre(nI);
  rd(in, kfState.data(), kfState.size()); rd(in, kfKind.data(), nKF); rd(in, mpPos.data(), mpPos.size());
  rd(in, eKF.data(), nE); rd(in, eMP.data(), nE); rd(in, eObs.data(), eObs.size()); rd(in, eRight.data(), nE); rd(in, eInv.data(), nE);
  rd(in, iKF1.data(), nI); rd(in, iKF2.data(), nI); rd(in, iPre.data(), nI);
  if (!in) { std::printf("short input\n"); return 2; }
  std::ofstream out(argv[2], std::ios::binary);
  {   // (1) the view-taking form
    std::vector<float> state = kfState, pos = mpPos;
    FullInertialBAView g;
    g.nKF = nKF; g.nMP = nMP; g.nE = nE; g.nI = nI; g.kfState = state.data(); g.kfKind = kfKind.data(); g.mpPos = pos.data();
    g.eKF = eKF.data(); g.eMP = eMP.data(); g.eObs = eObs.data(); g.eInvSigma2 = eInv.data(); g.iKF1 = iKF1.data(); g.iKF2 = iKF2.data(); g.iPre = iPre.data();
    g.fx = cam[0]; g.fy = cam[1]; g.cx = cam[2]; g.cy = cam[3]; g.mbf = cam[4];
    if (rig) { g.rig28 = rig28; g.eRight = eRight.data(); }
    std::memcpy(g.Tbc12, Tbc, sizeof Tbc); std::memcpy(g.bias6, bias6, sizeof bias6);
    bool flag = false;
    Optimizer::FullInertialBA(g, its, bInit, priors[0], priors[1], &flag, Optimizer::kLoopClosing);
    wr(out, state.data(), state.size()); wr(out, pos.data(), pos.size()); wr(out, g.bias6, 6); wr(out, g.stats, 4); wr(out, g.chi2, 2);
  }
  for (int run = 0; run < 2; ++run) {   // (2), (3) the reference signature on a mock map: keypoint i of a keyframe is its i-th edge of that camera
    FIMap map;
    GeometricCamera camL, camR;
    if (rig) { camL.mvParameters.assign(rig28, rig28 + 8); camR.mvParameters.assign(rig28 + 8, rig28 + 16); }
    std::vector<FIKeyFrame> kfs(nKF);
    std::vector<FIMapPoint> mps(nMP);
    std::vector<FIPreintegrated> pre(nI);
    for (int j = 0; j < nMP; ++j) { mps[j].mnId = j; mps[j].mWorldPos = Eigen::Vector3f(mpPos[3 * j], mpPos[3 * j + 1], mpPos[3 * j + 2]); map.mps.push_back(&mps[j]); }
    for (int k = 0; k < nKF; ++k) {
      FIKeyFrame& K = kfs[k];
      K.mnId = k;
      K.fx = cam[0]; K.fy = cam[1]; K.cx = cam[2]; K.cy = cam[3]; K.mbf = cam[4];
      if (rig) { K.mpCamera = &camL; K.mpCamera2 = &camR; K.NLeft = 0; for (int c = 0; c < 9; ++c) K.mTrl.R[c] = rig28[16 + c]; for (int c = 0; c < 3; ++c) K.mTrl.t[c] = rig28[25 + c]; }
      for (int c = 0; c < 9; ++c) K.mImuCalib.mTbc.R[c] = Tbc[c];
      for (int c = 0; c < 3; ++c) K.mImuCalib.mTbc.t[c] = Tbc[9 + c];
      const float* s = &kfState[(size_t)21 * k];
      for (int c = 0; c < 9; ++c) K.mRwb.m[c] = s[c];
      for (int c = 0; c < 3; ++c) { K.mOwb(c) = s[9 + c]; K.mVw(c) = s[12 + c]; }
      K.mImuBias = IMU::Bias(s[18], s[19], s[20], s[15], s[16], s[17]);
      K.bImu = kfKind[k] == 0;
      map.kfs.push_back(&K);
    }
    map.maxKFid = nKF - 1;
    for (int e = 0; e < nE; ++e) {
      FIKeyFrame& K = kfs[eKF[e]];
      FIMapPoint& P = mps[eMP[e]];
      cv::KeyPoint kp;
      kp.pt.x = eObs[3 * e]; kp.pt.y = eObs[3 * e + 1]; kp.octave = (int)K.mvInvLevelSigma2.size();
      K.mvInvLevelSigma2.push_back(eInv[e]);
      int left = -1, right = -1;
      const auto it = P.mObservations.find(&K);
      if (it != P.mObservations.end()) { left = std::get<0>(it->second); right = std::get<1>(it->second); }
      if (eRight[e]) { right = (int)K.mvKeysRight.size(); K.mvKeysRight.push_back(kp); }
      else { left = (int)K.mvKeysUn.size(); K.mvKeysUn.push_back(kp); K.mvuRight.push_back(rig ? -1.f : eObs[3 * e + 2]); }
      P.mObservations[&K] = std::make_tuple(left, right);
    }
    for (int i = 0; i < nI; ++i) {
      const morb_imu_preintegrated& r = iPre[i];
      FIPreintegrated& P = pre[i];
      P.dT = r.dT;
      auto m3 = [](Eigen::Matrix3f& M, const float* v) { for (int c = 0; c < 9; ++c) M.m[c] = v[c]; };
      auto v3 = [](Eigen::Vector3f& V, const float* v) { for (int c = 0; c < 3; ++c) V.v[c] = v[c]; };
      m3(P.dR, r.dR); v3(P.dV, r.dV); v3(P.dP, r.dP); m3(P.JRg, r.JRg); m3(P.JVg, r.JVg); m3(P.JVa, r.JVa); m3(P.JPg, r.JPg); m3(P.JPa, r.JPa);
      for (int c = 0; c < 225; ++c) P.C.m[c] = r.C[c];
      P.b = IMU::Bias(r.b[0], r.b[1], r.b[2], r.b[3], r.b[4], r.b[5]);
      for (int c = 0; c < 6; ++c) { P.Nga.d.v[c] = r.nga[c]; P.NgaWalk.d.v[c] = r.ngaWalk[c]; }
      v3(P.avgA, r.avgA); v3(P.avgW, r.avgW);
      kfs[iKF2[i]].mpImuPreintegrated = &P; kfs[iKF2[i]].mPrevKF = &kfs[iKF1[i]];
    }
    bool mbStopGBA = false;
    if (run == 0) Optimizer::FullInertialBA(&map, its, false, 0, NULL, bInit, priors[0], priors[1]);
    else Optimizer::FullInertialBA(&map, its, false, 5, &mbStopGBA, bInit, priors[0], priors[1]);
    for (int k = 0; k < nKF; ++k) {
      FIKeyFrame& K = kfs[k];
      const int counts[4] = {K.nSetPose, K.nSetVelocity, K.nSetNewBias, (int)K.mnBAGlobalForKF};
      const Sophus::SE3f& T = run ? K.mTcwGBA : K.mTcw;
      const Eigen::Vector3f& v = run ? K.mVwbGBA : K.mVw;
      const IMU::Bias& b = run ? K.mBiasGBA : K.mImuBias;
      const float bias[6] = {b.bwx, b.bwy, b.bwz, b.bax, b.bay, b.baz};
      wr(out, counts, 4); wr(out, T.R, 9); wr(out, T.t, 3); wr(out, v.v, 3); wr(out, bias, 6);
    }
    for (int j = 0; j < nMP; ++j) { const int c[2] = {mps[j].nUpdates, (int)mps[j].mnBAGlobalForKF}; wr(out, c, 2); wr(out, run ? mps[j].mPosGBA.v : mps[j].mWorldPos.v, 3); }
    for (int i = 0; i < nI; ++i) wr(out, &pre[i].nSetNewBias, 1);
    wr(out, &map.changes, 1);
  }
  std::printf("full inertial ba adapter ok\n");
  return out ? 0 : 1;
}
