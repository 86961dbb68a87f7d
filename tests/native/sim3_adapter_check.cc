// Drives Optimizer::OptimizeSim3 in the reference's signature (the member template of include/morb/Optimizer_reference.h) on the GPU with
// the mock KeyFrame / MapPoint of tests/native/mock_ref and the g2o::Sim3 / Eigen mocks of tests/native/mock_sim3.  tests/test_sim3_gpu.py
// writes one problem per file and compares what this program writes with the Python path (morb_optimize_sim3_batch on the same data).
//   in:  int32 N, N2, camKind1, camKind2, fixScale, allPoints; float th2, cam1[8], cam2[8], T1w[12], T2w[12], invLevel[8]; double S12[8];
//        per KF1 feature: uint8 entry, int32 i2, float Xw1[3], Xw2[3], kp1 x y, int32 octave1, int32 mnTrackScaleLevel of pMP2;
//        per KF2 feature: float x y, int32 octave.
//   out: int32 return value, uint8 vpMatches1[i] != NULL (N), double g2oS12 (qx qy qz qw tx ty tz s), int32 mAcumHessian state
//        (1 all zero, 0 untouched, -1 anything else).
#include <cstdio>
#include <memory>
#include <vector>

#include "KeyFrame.h"       // tests/native/mock_ref
#include "MapPoint.h"
#include "g2o_sim3_mock.h"  // tests/native/mock_sim3
#include "Optimizer.h"      // include/morb

namespace ORB_SLAM3 { std::mutex MapPoint::mGlobalMutex; }
using namespace ORB_SLAM3;

template <class T> static bool rd(FILE* f, T* p, size_t n = 1) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int N, N2, kind1, kind2, fix, all;
  float th2, cam1[8], cam2[8], T1[12], T2[12], invLevel[8];
  double S[8];
  bool ok = rd(f, &N) && rd(f, &N2) && rd(f, &kind1) && rd(f, &kind2) && rd(f, &fix) && rd(f, &all) && rd(f, &th2) && rd(f, cam1, 8) &&
            rd(f, cam2, 8) && rd(f, T1, 12) && rd(f, T2, 12) && rd(f, invLevel, 8) && rd(f, S, 8);
  if (!ok || N < 0 || N2 < 0) return 3;
  GeometricCamera c1, c2;
  c1.mvParameters.assign(cam1, cam1 + (kind1 ? 8 : 4));
  c2.mvParameters.assign(cam2, cam2 + (kind2 ? 8 : 4));
  KeyFrame kf1, kf2;
  for (KeyFrame* k : {&kf1, &kf2}) k->mvInvLevelSigma2.assign(invLevel, invLevel + 8);
  kf1.mpCamera = &c1; kf2.mpCamera = &c2;
  for (int k = 0; k < 9; ++k) { kf1.mTcw.R[k] = T1[k]; kf2.mTcw.R[k] = T2[k]; }
  for (int k = 0; k < 3; ++k) { kf1.mTcw.t[k] = T1[9 + k]; kf2.mTcw.t[k] = T2[9 + k]; }
  kf1.N = N; kf2.N = N2;
  kf1.mvKeysUn.resize(N); kf1.mvpMapPoints.assign(N, nullptr);
  std::vector<std::unique_ptr<MapPoint>> pts;
  std::vector<MapPoint*> vpMatches1(N, nullptr);
  for (int i = 0; i < N; ++i) {
    uint8_t e; int i2, oct1, level2; float X1[3], X2[3], kp[2];
    if (!(rd(f, &e) && rd(f, &i2) && rd(f, X1, 3) && rd(f, X2, 3) && rd(f, kp, 2) && rd(f, &oct1) && rd(f, &level2))) return 3;
    kf1.mvKeysUn[i].pt.x = kp[0]; kf1.mvKeysUn[i].pt.y = kp[1]; kf1.mvKeysUn[i].octave = oct1;
    if (e & 2) {
      pts.emplace_back(new MapPoint);
      MapPoint* p1 = pts.back().get();
      p1->mWorldPos = Eigen::Vector3f(X1[0], X1[1], X1[2]);
      p1->mbBad = (e & 4) != 0;
      kf1.mvpMapPoints[i] = p1;
    }
    if (e & 1) {
      pts.emplace_back(new MapPoint);
      MapPoint* p2 = pts.back().get();
      p2->mWorldPos = Eigen::Vector3f(X2[0], X2[1], X2[2]);
      p2->mbBad = (e & 8) != 0;
      p2->mnTrackScaleLevel = level2;
      if (i2 >= 0) p2->mObservations[&kf2] = std::make_tuple(i2, -1);
      vpMatches1[i] = p2;
    }
  }
  kf2.mvKeysUn.resize(N2);
  for (int j = 0; j < N2; ++j) {
    float kp[2]; int oct;
    if (!(rd(f, kp, 2) && rd(f, &oct))) return 3;
    kf2.mvKeysUn[j].pt.x = kp[0]; kf2.mvKeysUn[j].pt.y = kp[1]; kf2.mvKeysUn[j].octave = oct;
  }
  fclose(f);
  Eigen::Vector3d t;
  for (int k = 0; k < 3; ++k) t(k) = S[4 + k];
  g2o::Sim3 gS(Eigen::Quaterniond(S[3], S[0], S[1], S[2]), t, S[7]);
  Eigen::Matrix<double, 7, 7> H;
  for (double& v : H.m) v = 7.0;
  const int ret = Optimizer::OptimizeSim3(&kf1, &kf2, vpMatches1, gS, th2, fix != 0, H, all != 0);
  int zero = 1, untouched = 1;
  for (double v : H.m) { zero &= v == 0.0; untouched &= v == 7.0; }
  const int hstate = zero ? 1 : untouched ? 0 : -1;
  const double out[8] = {gS.rotation().x(), gS.rotation().y(), gS.rotation().z(), gS.rotation().w(), gS.translation()(0), gS.translation()(1),
                         gS.translation()(2), gS.scale()};
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 4;
  fwrite(&ret, 4, 1, o);
  for (int i = 0; i < N; ++i) { const uint8_t k = vpMatches1[i] != nullptr; fwrite(&k, 1, 1, o); }
  fwrite(out, 8, 8, o);
  fwrite(&hstate, 4, 1, o);
  fclose(o);
  printf("ret %d hessian %d\n", ret, hstate);
  return 0;
}
