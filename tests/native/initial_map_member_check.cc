// The reference-typed Optimizer::GlobalBundleAdjustemnt / BundleAdjustment members of include/morb/Optimizer.h on a mock map
// (tests/native/mock_initial_map), with the argument list of the call site in Tracking::CreateInitialMapMonocular:
//   Optimizer::GlobalBundleAdjustemnt(mpAtlas->GetCurrentMap(), 20)
// `initial_map_member_check refusals`: a map of three keyframes and a map whose point carries a stereo observation are refused with
// std::runtime_error before anything reaches the device.  The CPU suite also looks for the two members in the program.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "initial_map_mock.h"
#include "Optimizer.h"

using namespace ORB_SLAM3;

template void Optimizer::GlobalBundleAdjustemnt<IMMap>(IMMap*, int, bool*, unsigned long, bool);
template void Optimizer::BundleAdjustment<IMKeyFrame, IMMapPoint>(const std::vector<IMKeyFrame*>&, const std::vector<IMMapPoint*>&, int, bool*, unsigned long,
                                                                  bool);

struct Scene {
  IMMap map;
  std::vector<IMKeyFrame> kfs;
  std::vector<IMMapPoint> mps;
  GeometricCamera cam;
  Scene(int nKF, int nMP) : kfs(nKF), mps(nMP) {
    cam.mvParameters = {458.f, 457.f, 367.f, 248.f};
    for (int k = 0; k < nKF; ++k) {
      IMKeyFrame& K = kfs[k];
      K.mnId = k; K.mpMap = &map; K.mpCamera = &cam; K.mnScaleLevels = 2;
      K.mvScaleFactors = {1.f, 1.2f}; K.mvLevelSigma2 = {1.f, 1.44f}; K.mvInvLevelSigma2 = {1.f, 1.f / 1.44f};
      K.mvKeysUn.resize(nMP); K.mvuRight.assign(nMP, -1.f); K.N = nMP;
      for (int i = 0; i < nMP; ++i) { K.mvKeysUn[i].pt.x = 300.f + 7 * i + 3 * k; K.mvKeysUn[i].pt.y = 200.f + 5 * i; }
      if (k) K.mTcw.t[0] = 0.3f * k;
      map.keyframes.push_back(&K);
    }
    for (int i = 0; i < nMP; ++i) {
      mps[i].mnId = i; mps[i].mpMap = &map;
      mps[i].mWorldPos = Eigen::Vector3f(0.1f * i, 0.05f * i, 5.f);
      for (int k = 0; k < nKF; ++k) mps[i].AddObservation(&kfs[k], i);
      map.points.push_back(&mps[i]);
    }
    map.initKF = 0;
  }
};

int main(int argc, char** argv) {
  if (argc < 2 || std::strcmp(argv[1], "refusals")) { std::printf("usage: %s refusals\n", argv[0]); return 2; }
  {
    Scene s(3, 12);
    bool thrown = false;
    try { Optimizer::GlobalBundleAdjustemnt(&s.map, 20); } catch (const std::runtime_error& e) { thrown = true; std::printf("three keyframes refused: %s\n", e.what()); }
    if (!thrown) { std::printf("a map of three keyframes was accepted\n"); return 1; }
  }
  {
    Scene s(2, 12);
    s.kfs[1].mvuRight[4] = 250.f;
    bool thrown = false;
    try { Optimizer::GlobalBundleAdjustemnt(&s.map, 20); } catch (const std::runtime_error& e) { thrown = true; std::printf("stereo observation refused: %s\n", e.what()); }
    if (!thrown) { std::printf("a stereo observation was accepted\n"); return 1; }
  }
  return 0;
}
