// Optimizer::BundleAdjustment(InitialMapView&, ...) and Optimizer::CreateInitialMapMonocular(InitialMapView&) of include/morb/Optimizer.h on one
// problem read from a file, and the reference-typed GlobalBundleAdjustemnt on a mock map built from the same problem (both nLoopKF cases).
// Run as `initial_map_adapter_check <in.bin> <out.bin>`; tests/test_initial_map_adapter_gpu.py compares what it dumps with the C entry.
// in.bin: int n1, n2, nlevels, kb8; float cam8[8], scaleFactors[16], levelSigma2[16], T21[12]; kp1 [n1][3], kp2 [n2][3] (x, y, octave) float;
// int matches12[n1]; uint8 triangulated[n1]; float P3D[n1][3].
#include <cstdio>
#include <fstream>
#include <vector>

#include "initial_map_mock.h"
#include "Optimizer.h"

using namespace ORB_SLAM3;

template <class T> static void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), n * sizeof(T)); }
template <class T> static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), n * sizeof(T)); }

static void dump(std::ofstream& f, const InitialMapView& v) {
  const int head[5] = {v.status, v.nPoints, v.outerIterations, v.lmTrials, v.stopSeen ? 1 : 0};
  wr(f, head, 5); wr(f, v.Tcw2, 12); wr(f, v.chi2, 2); wr(f, &v.medianDepth, 1);
  wr(f, v.mpPos.data(), v.mpPos.size()); wr(f, v.mpNormal.data(), v.mpNormal.size()); wr(f, v.mpDist.data(), v.mpDist.size()); wr(f, v.hasMP.data(), v.hasMP.size());
}

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: %s in.bin out.bin\n", argv[0]); return 2; }
  std::ifstream in(argv[1], std::ios::binary);
  int hd[4];
  rd(in, hd, 4);
  const int n1 = hd[0], n2 = hd[1];
  InitialMapView v;
  v.n1 = n1; v.n2 = n2; v.nlevels = hd[2]; v.kb8 = hd[3] != 0;
  rd(in, v.cam8, 8); rd(in, v.scaleFactors, 16); rd(in, v.levelSigma2, 16); rd(in, v.T21, 12);
  std::vector<float> k1((size_t)n1 * 3), k2((size_t)n2 * 3), p3d((size_t)n1 * 3);
  std::vector<int> m12(n1);
  std::vector<uint8_t> tri(n1);
  rd(in, k1.data(), k1.size()); rd(in, k2.data(), k2.size()); rd(in, m12.data(), n1); rd(in, tri.data(), n1); rd(in, p3d.data(), p3d.size());
  if (!in) { std::printf("short input\n"); return 2; }
  std::vector<morb_keypoint> keys1(n1), keys2(n2);
  for (int i = 0; i < n1; ++i) { keys1[i] = morb_keypoint{k1[3 * i], k1[3 * i + 1], 31.f, 0.f, 0.f, (int)k1[3 * i + 2], -1}; }
  for (int i = 0; i < n2; ++i) { keys2[i] = morb_keypoint{k2[3 * i], k2[3 * i + 1], 31.f, 0.f, 0.f, (int)k2[3 * i + 2], -1}; }
  v.keysUn1 = keys1.data(); v.keysUn2 = keys2.data(); v.matches12 = m12.data(); v.triangulated = tri.data(); v.P3D = p3d.data();
  std::ofstream out(argv[2], std::ios::binary);
  // (1) the bare bundle adjustment: 10 iterations, not robust, no scaling
  v.depthScale = 0.f; v.minTracked = 0;
  Optimizer::BundleAdjustment(v, 10, false);
  dump(out, v);
  // (2) the whole numeric part, IMU-monocular
  const bool good = Optimizer::CreateInitialMapMonocular(v, true);
  dump(out, v);
  const int g = good ? 1 : 0;
  wr(out, &g, 1);
  // (3) the reference signature on a mock map of the same problem, nLoopKF = 0 (the map's own origin), then nLoopKF = 7
  for (unsigned long loopKF : {0ul, 7ul}) {
    IMMap map;
    GeometricCamera cam;
    cam.mvParameters.assign(v.cam8, v.cam8 + (v.kb8 ? 8 : 4));
    std::vector<IMKeyFrame> kfs(2);
    for (int k = 0; k < 2; ++k) {
      IMKeyFrame& K = kfs[k];
      const std::vector<morb_keypoint>& keys = k ? keys2 : keys1;
      K.mnId = k; K.mpMap = &map; K.mpCamera = &cam; K.mnScaleLevels = v.nlevels;
      K.mvScaleFactors.assign(v.scaleFactors, v.scaleFactors + v.nlevels); K.mvLevelSigma2.assign(v.levelSigma2, v.levelSigma2 + v.nlevels);
      K.mvKeysUn.resize(keys.size()); K.mvuRight.assign(keys.size(), -1.f);
      for (size_t i = 0; i < keys.size(); ++i) { K.mvKeysUn[i].pt.x = keys[i].x; K.mvKeysUn[i].pt.y = keys[i].y; K.mvKeysUn[i].octave = keys[i].octave; }
      map.keyframes.push_back(&K);
    }
    for (int k = 0; k < 9; ++k) kfs[1].mTcw.R[k] = v.T21[k];
    for (int k = 0; k < 3; ++k) kfs[1].mTcw.t[k] = v.T21[9 + k];
    std::vector<IMMapPoint> mps(n1);
    for (int i = 0; i < n1; ++i) {
      if (m12[i] < 0 || m12[i] >= n2 || !tri[i]) continue;
      mps[i].mnId = i; mps[i].mpMap = &map; mps[i].mWorldPos = Eigen::Vector3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
      mps[i].AddObservation(&kfs[0], i); mps[i].AddObservation(&kfs[1], m12[i]);
      map.points.push_back(&mps[i]);
    }
    map.initKF = 0;
    Optimizer::GlobalBundleAdjustemnt(&map, 20, (bool*)nullptr, loopKF);
    const Sophus::SE3f T = loopKF == 0 ? kfs[1].mTcw : kfs[1].mTcwGBA;
    wr(out, T.R, 9); wr(out, T.t, 3);
    std::vector<float> pos((size_t)n1 * 3, 0.f);
    std::vector<int> upd(n1, 0);
    for (int i = 0; i < n1; ++i) {
      const Eigen::Vector3f X = loopKF == 0 ? mps[i].mWorldPos : mps[i].mPosGBA;
      for (int k = 0; k < 3; ++k) pos[3 * i + k] = X(k);
      upd[i] = mps[i].nUpdates * 100 + (int)mps[i].mnBAGlobalForKF;
    }
    wr(out, pos.data(), pos.size()); wr(out, upd.data(), n1);
    const int marks[2] = {(int)kfs[0].mnBAGlobalForKF, (int)kfs[1].mnBAGlobalForKF};
    wr(out, marks, 2);
  }
  return out ? 0 : 1;
}
