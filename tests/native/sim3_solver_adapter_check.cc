// Drives ORB_SLAM3::Sim3Solver in the reference's signature (include/morb/Sim3Solver.h) on the GPU with the mock KeyFrame / MapPoint of
// tests/native/mock_ref and the Matrix4f of tests/native/mock_sim3_solver, after srand(seed), three ways: find(), LoopClosing's
// `while (!bConverge && !bNoMore) iterate(20, .., bConverge)` and one four-argument iterate(20, ..).  tests/test_sim3_solver_adapter_gpu.py
// writes one problem per file and compares what this program writes with the CPU oracle on the same rand() stream.
//   in:  int32 N1, kind1, kind2, fixScale, seed, minInliers, maxIterations, useKFm, rig1; double probability;
//        float cam1[8], cam2[8], T1w[12], T2w[12], levelSigma2[8];
//        per KF1 feature: uint8 entry (bits as morb_sim3_solver_batch), float Xw1[3], Xw2[3], int32 octave1, octave2, kfm (0 pKF2, 1 pKF3).
//   A feature's keypoint sits at its own index in KF1 and in its pKFm; the other keyframe holds a keypoint with a different octave there,
//   as does KF1's mvKeysUn beyond NLeft when rig1 (the feature's own row is mvKeysRight[i - NLeft]).
//   out per drive (find, loop, iterate4): int32 calls, bConverge, bNoMore, nInliers; uint8 vbInliers[N1]; float returned[16], T[16], R[9],
//   t[3], s.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "KeyFrame.h"           // tests/native/mock_ref
#include "MapPoint.h"
#include "loop_closing_mock.h"  // tests/native/mock_sim3_solver
#include "Sim3Solver.h"         // include/morb

namespace ORB_SLAM3 { std::mutex MapPoint::mGlobalMutex; }
using namespace ORB_SLAM3;

template <class T> static bool rd(FILE* f, T* p, size_t n = 1) { return fread(p, sizeof(T), n, f) == n; }

struct Out {
  int calls = 0, conv = 0, noMore = 0, nIn = 0;
  std::vector<uint8_t> vb;
  float ret[16], T[16], R[9], t[3], s;
};

static void finish(Out& o, Sim3Solver& S, const Eigen::Matrix4f& ret, const std::vector<bool>& vb, int n) {
  for (int i = 0; i < 16; ++i) o.ret[i] = ret(i / 4, i % 4);
  const Eigen::Matrix4f T = S.GetEstimatedTransformation();
  const Eigen::Matrix3f R = S.GetEstimatedRotation();
  const Eigen::Vector3f t = S.GetEstimatedTranslation();
  for (int i = 0; i < 16; ++i) o.T[i] = T(i / 4, i % 4);
  for (int i = 0; i < 9; ++i) o.R[i] = R(i / 3, i % 3);
  for (int i = 0; i < 3; ++i) o.t[i] = t(i);
  o.s = S.GetEstimatedScale();
  o.vb.assign(n, 0);
  for (int i = 0; i < n && i < (int)vb.size(); ++i) o.vb[i] = vb[i] ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int N, kind1, kind2, fix, seed, minIn, maxIts, useKFm, rig1;
  double prob;
  float cam1[8], cam2[8], T1[12], T2[12], lev[8];
  bool ok = rd(f, &N) && rd(f, &kind1) && rd(f, &kind2) && rd(f, &fix) && rd(f, &seed) && rd(f, &minIn) && rd(f, &maxIts) && rd(f, &useKFm) &&
            rd(f, &rig1) && rd(f, &prob) && rd(f, cam1, 8) && rd(f, cam2, 8) && rd(f, T1, 12) && rd(f, T2, 12) && rd(f, lev, 8);
  if (!ok || N < 0) return 3;
  GeometricCamera c1, c2;
  c1.mvParameters.assign(cam1, cam1 + (kind1 ? 8 : 4));
  c2.mvParameters.assign(cam2, cam2 + (kind2 ? 8 : 4));
  KeyFrame kf1, kf2, kf3;
  for (KeyFrame* k : {&kf1, &kf2, &kf3}) {
    k->mvLevelSigma2.assign(lev, lev + 8);
    k->N = N;
    k->mvKeysUn.resize(N);
  }
  kf1.mpCamera = &c1; kf2.mpCamera = &c2; kf3.mpCamera = &c2;
  for (int k = 0; k < 9; ++k) { kf1.mTcw.R[k] = T1[k]; kf2.mTcw.R[k] = T2[k]; kf3.mTcw.R[k] = T2[k]; }
  for (int k = 0; k < 3; ++k) { kf1.mTcw.t[k] = T1[9 + k]; kf2.mTcw.t[k] = T2[9 + k]; kf3.mTcw.t[k] = T2[9 + k]; }
  if (rig1) {
    kf1.NLeft = N / 2;
    kf1.mvKeysRight.resize(N - N / 2);
  }
  kf1.mvpMapPoints.assign(N, nullptr);
  std::vector<std::unique_ptr<MapPoint>> pts;
  std::vector<MapPoint*> vpMatched12(N, nullptr);
  std::vector<KeyFrame*> vpKFm;
  if (useKFm) vpKFm.assign(N, &kf2);
  for (int i = 0; i < N; ++i) {
    uint8_t e;
    float X1[3], X2[3];
    int oct1, oct2, kfm;
    if (!(rd(f, &e) && rd(f, X1, 3) && rd(f, X2, 3) && rd(f, &oct1) && rd(f, &oct2) && rd(f, &kfm))) return 3;
    const int wrong1 = (oct1 + 3) % 8, wrong2 = (oct2 + 5) % 8;
    if (rig1 && i >= kf1.NLeft) {
      kf1.mvKeysRight[i - kf1.NLeft].octave = oct1;
      kf1.mvKeysUn[i].octave = wrong1;
    } else {
      kf1.mvKeysUn[i].octave = oct1;
    }
    KeyFrame* pKFm = kfm ? &kf3 : &kf2;
    KeyFrame* other = kfm ? &kf2 : &kf3;
    pKFm->mvKeysUn[i].octave = oct2;
    other->mvKeysUn[i].octave = wrong2;
    if (useKFm) vpKFm[i] = pKFm;
    if (e & 2) {
      pts.emplace_back(new MapPoint);
      MapPoint* p1 = pts.back().get();
      p1->mWorldPos = Eigen::Vector3f(X1[0], X1[1], X1[2]);
      p1->mbBad = (e & 4) != 0;
      if (!(e & 16)) p1->mObservations[&kf1] = std::make_tuple(i, -1);
      kf1.mvpMapPoints[i] = p1;
    }
    if (e & 1) {
      pts.emplace_back(new MapPoint);
      MapPoint* p2 = pts.back().get();
      p2->mWorldPos = Eigen::Vector3f(X2[0], X2[1], X2[2]);
      p2->mbBad = (e & 8) != 0;
      if (!(e & 32)) p2->mObservations[pKFm] = std::make_tuple(i, -1);
      vpMatched12[i] = p2;
    }
  }
  fclose(f);
  const bool bFix = fix != 0;
  Out o[3];
  {   // find()
    srand(seed);
    Sim3Solver S = useKFm ? Sim3Solver(&kf1, &kf2, vpMatched12, bFix, vpKFm) : Sim3Solver(&kf1, &kf2, vpMatched12, bFix);
    S.SetRansacParameters(prob, minIn, maxIts);
    std::vector<bool> vb;
    int nIn = -1;
    const Eigen::Matrix4f ret = S.find(vb, nIn);
    o[0].calls = 1; o[0].nIn = nIn; o[0].conv = S.state().converged; o[0].noMore = S.state().noMore;
    finish(o[0], S, ret, vb, N);
  }
  {   // LoopClosing.cc:715-722
    srand(seed);
    Sim3Solver S = useKFm ? Sim3Solver(&kf1, &kf2, vpMatched12, bFix, vpKFm) : Sim3Solver(&kf1, &kf2, vpMatched12, bFix);
    S.SetRansacParameters(prob, minIn, maxIts);
    bool bNoMore = false, bConverge = false;
    std::vector<bool> vb;
    int nIn = -1;
    Eigen::Matrix4f ret;
    while (!bConverge && !bNoMore) {
      ret = S.iterate(20, bNoMore, vb, nIn, bConverge);
      o[1].calls++;
    }
    o[1].nIn = nIn; o[1].conv = bConverge; o[1].noMore = bNoMore;
    finish(o[1], S, ret, vb, N);
  }
  {   // one iterate(20, bNoMore, vbInliers, nInliers)
    srand(seed);
    Sim3Solver S = useKFm ? Sim3Solver(&kf1, &kf2, vpMatched12, bFix, vpKFm) : Sim3Solver(&kf1, &kf2, vpMatched12, bFix);
    S.SetRansacParameters(prob, minIn, maxIts);
    bool bNoMore = false;
    std::vector<bool> vb;
    int nIn = -1;
    const Eigen::Matrix4f ret = S.iterate(20, bNoMore, vb, nIn);
    o[2].calls = 1; o[2].nIn = nIn; o[2].conv = S.state().converged; o[2].noMore = bNoMore;
    finish(o[2], S, ret, vb, N);
  }
  FILE* w = fopen(argv[2], "wb");
  if (!w) return 4;
  for (Out& x : o) {
    const int hdr[4] = {x.calls, x.conv, x.noMore, x.nIn};
    fwrite(hdr, 4, 4, w);
    fwrite(x.vb.data(), 1, N, w);
    fwrite(x.ret, 4, 16, w); fwrite(x.T, 4, 16, w); fwrite(x.R, 4, 9, w); fwrite(x.t, 4, 3, w); fwrite(&x.s, 4, 1, w);
  }
  fclose(w);
  printf("find %d/%d loop %d calls %d/%d iterate4 %d/%d\n", o[0].conv, o[0].nIn, o[1].calls, o[1].conv, o[1].nIn, o[2].conv, o[2].nIn);
  return 0;
}
