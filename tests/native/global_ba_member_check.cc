// The reference-typed Optimizer::WholeMapBundleAdjustment of include/morb/Optimizer_reference.h on a mock map (tests/native/mock_global_ba), and
// Optimizer::GlobalBundleAdjustemnt with the five arguments of LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:2302) under
// MORB_WHOLE_MAP_BUNDLE_ADJUSTMENT.  Host side only: the C entries the members reach are STUBS defined here — morb_bundle_adjustment_fisheye
// checks the flattened graph against the edge list written by hand below and returns canned results — so the program needs neither the library
// nor a GPU and runs under -fsanitize=address,undefined.  Checked: the flattening alone (morb_glue::flatten_whole_map: a bad keyframe, a bad
// point, a keyframe outside vpKFs, a point without an edge, a rig keyframe with left and right observations, keyframes handed over out of
// order), and the write-back for both nLoopKF cases.
#define MORB_WHOLE_MAP_BUNDLE_ADJUSTMENT
#include <cstdio>
#include <cstring>
#include <vector>

#include "global_ba_mock.h"
#include "Optimizer.h"

using namespace ORB_SLAM3;
std::mutex ORB_SLAM3::MapPoint::mGlobalMutex;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// LoopClosing.cc:2302's overload, instantiated whole: Optimizer::GlobalBundleAdjustemnt(pActiveMap, 10, &mbStopGBA, nLoopKF, false)
template void Optimizer::GlobalBundleAdjustemnt<GBMap>(GBMap*, int, bool*, unsigned long, bool);

struct Expect { std::vector<float> kfPose, mpPos, eObs2, eInv; std::vector<uint8_t> kfFixed, eRight; std::vector<int> eKF, eMP; } g_expect;
static int g_calls = 0, g_bad = 0, g_its = 0, g_robust = -1;
extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
int morb_optimizer_create(morb_optimizer** out, int) { static int token; *out = reinterpret_cast<morb_optimizer*>(&token); return MORB_OK; }
int morb_optimizer_set_exact_order(morb_optimizer*, int) { return MORB_OK; }
const char* morb_last_error(void) { return "stub"; }
int morb_bundle_adjustment_fisheye(morb_optimizer*, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos, int nE, const int* eKF,
                                   const int* eMP, const float* eObs2, const uint8_t* eRight, const float* eInvSigma2, const float* camL8,
                                   const float* camR8, const float* Trl7, int nIterations, int bRobust, const uint8_t* stopFlag, int* stats4, double* chi2) {
  ++g_calls; g_its = nIterations; g_robust = bRobust;
  const Expect& x = g_expect;
  auto same = [](const auto& v, const auto* p, size_t n) { return v.size() == n && (n == 0 || std::memcmp(v.data(), p, n * sizeof(v[0])) == 0); };
  if (!same(x.kfPose, kfPose, (size_t)nKF * 7) || !same(x.kfFixed, kfFixed, nKF) || !same(x.mpPos, mpPos, (size_t)nMP * 3) || !same(x.eKF, eKF, nE) ||
      !same(x.eMP, eMP, nE) || !same(x.eObs2, eObs2, (size_t)nE * 2) || !same(x.eRight, eRight, nE) || !same(x.eInv, eInvSigma2, nE) ||
      camL8[0] != 190.f || camR8[0] != 191.f || Trl7[3] != 1.f || Trl7[4] != -0.1f || !stopFlag || *stopFlag)
    ++g_bad;
  for (int i = 0; i < nKF; ++i) if (!kfFixed[i]) for (int c = 0; c < 7; ++c) kfPose[7 * i + c] = 100.f + 7 * i + c;   // (fixed keyframes keep their bytes)
  for (int i = 0; i < nMP * 3; ++i) mpPos[i] = 200.f + i;
  const int s[4] = {3, 4, nKF - 1, nKF};
  std::memcpy(stats4, s, sizeof s);
  chi2[0] = 2; chi2[1] = 1;
  return MORB_OK;
}
int morb_bundle_adjustment(morb_optimizer*, int, float*, const uint8_t*, int, float*, int, const int*, const int*, const float*, const float*, float, float,
                           float, float, float, int, int, const uint8_t*, int*, double*) { ++g_bad; return MORB_ERR_INVALID; }
// what the initial-map branch of BundleAdjustment<KF, MP> links against; this map is refused by that branch before it reaches any of them
static int unreachable() { ++g_bad; return MORB_ERR_INVALID; }
hipError_t hipMalloc(void**, size_t) { ++g_bad; return hipErrorInvalidValue; }
hipError_t hipHostMalloc(void**, size_t, unsigned int) { ++g_bad; return hipErrorInvalidValue; }
hipError_t hipFree(void*) { return hipSuccess; }
hipError_t hipHostFree(void*) { return hipSuccess; }
hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind, hipStream_t) { ++g_bad; return hipErrorInvalidValue; }
hipError_t hipStreamSynchronize(hipStream_t) { ++g_bad; return hipErrorInvalidValue; }
void* morb_optimizer_stream(const morb_optimizer*) { ++g_bad; return nullptr; }
int morb_create_initial_map_monocular_batch(morb_optimizer*, const morb_frame_params*, const float*, int, int, int, const int*, const int*, const int*,
                                            const morb_keypoint*, const int*, const int*, const float*, const float*, const uint8_t*, int, int, float, int,
                                            const unsigned char*, int*, float*, float*, float*, float*, uint8_t*, int*, double*, float*, void*) { return unreachable(); }
}

// Six keyframes on a KannalaBrandt8 rig with ids 20 .. 25, handed over as 22, 20, 21, 23, 24 (25 stays outside vpKFs); 21 is bad; 20 is the
// map's initial keyframe.  Seven points.
struct Scene {
  GBMap map;
  GeometricCamera camL, camR;
  std::vector<GBKeyFrame> kfs;
  std::vector<GBMapPoint> mps;
  Scene() : kfs(6), mps(7) {
    camL.mvParameters = {190.f, 190.5f, 254.f, 256.f, 0.003f, 0.0007f, -0.002f, 0.0002f};
    camR.mvParameters = {191.f, 191.5f, 252.f, 255.f, 0.003f, 0.0017f, -0.003f, 0.0003f};
    for (int k = 0; k < 6; ++k) {
      GBKeyFrame& K = kfs[k];
      K.mnId = 20 + k; K.mpMap = &map; K.mpCamera = &camL; K.mpCamera2 = &camR;
      K.mvInvLevelSigma2 = {1.f, 0.5f, 0.25f};
      K.NLeft = 6; K.N = 10; K.mvKeysUn.resize(6); K.mvuRight.assign(6, -1.f); K.mvKeysRight.resize(12);   // (mvKeysRight.size() > N: :226's test passes for 6 .. 9)
      for (int i = 0; i < 6; ++i) { K.mvKeysUn[i].pt.x = 100.f * k + i; K.mvKeysUn[i].pt.y = 50.f * k + 2 * i; K.mvKeysUn[i].octave = i % 3; }
      for (int i = 0; i < 12; ++i) { K.mvKeysRight[i].pt.x = 1000.f + 100.f * k + i; K.mvKeysRight[i].pt.y = 2000.f + 50.f * k + i; K.mvKeysRight[i].octave = (i + 1) % 3; }
      const float q[4] = {0.01f * k, 0.02f, 0.03f, 0.99f};
      for (int c = 0; c < 4; ++c) K.mTcw.q[c] = q[c];
      for (int c = 0; c < 3; ++c) K.mTcw.t[c] = 0.5f * k + c;
      K.mTrl.t[0] = -0.1f;
    }
    kfs[1].mbBad = true;
    map.initKF = 20; map.origin = &kfs[0];
    map.keyframes = {&kfs[2], &kfs[0], &kfs[1], &kfs[3], &kfs[4]};
    for (int j = 0; j < 7; ++j) { mps[j].mnId = j; mps[j].mpMap = &map; mps[j].mWorldPos = Eigen::Vector3f(1.f + j, 2.f + j, 5.f + j); map.points.push_back(&mps[j]); }
    mps[2].mbBad = true;
    auto see = [&](int k, int j, int left, int right) { mps[j].AddObservation(&kfs[k], left, right); };
    see(0, 0, 1, -1); see(2, 0, 2, 7); see(3, 0, 3, -1);   // point 0: left in 20, left + right in 22, left in 23
    see(2, 1, 4, -1); see(1, 1, 0, -1); see(5, 1, 0, 6);   // point 1: keyframe 22; the bad keyframe and the one outside vpKFs give no edge
    see(0, 2, 5, -1); see(3, 2, 5, -1);                    // the bad point
    see(1, 3, 1, -1); see(5, 3, 1, -1);                    // point 3: only seen by keyframes that do not enter: no edge, left out
    see(4, 4, -1, 8); see(0, 4, 0, 9);                     // point 4: the right camera alone in 24; left + right in 20
    see(3, 5, 0, 13);                                      // point 5: a right index beyond mvKeysRight: the left edge only (:226)
    // point 6: nobody observes it
  }
};

static void expect_of(Scene& s) {
  Expect& x = g_expect;
  x = Expect();
  for (int k : {0, 2, 3, 4}) { for (int c = 0; c < 4; ++c) x.kfPose.push_back(s.kfs[k].mTcw.q[c]); for (int c = 0; c < 3; ++c) x.kfPose.push_back(s.kfs[k].mTcw.t[c]); }
  x.kfFixed = {1, 0, 0, 0};
  for (int j : {0, 1, 4, 5}) for (int c = 0; c < 3; ++c) x.mpPos.push_back(s.mps[j].mWorldPos(c));
  // vertex, point row, keyframe, keypoint (an index into mvKeysRight when right); observations within a point come by keyframe address
  const int edges[8][5] = {{0, 0, 0, 1, 0}, {1, 0, 2, 2, 0}, {1, 0, 2, 1, 1}, {2, 0, 3, 3, 0}, {1, 1, 2, 4, 0}, {0, 2, 0, 0, 0}, {0, 2, 0, 3, 1}, {3, 2, 4, 2, 1}};
  for (const auto& e : edges) {
    x.eKF.push_back(e[0]); x.eMP.push_back(e[1]); x.eRight.push_back((uint8_t)e[4]);
    const cv::KeyPoint& kp = e[4] ? s.kfs[e[2]].mvKeysRight[e[3]] : s.kfs[e[2]].mvKeysUn[e[3]];
    x.eObs2.push_back(kp.pt.x); x.eObs2.push_back(kp.pt.y);
    x.eInv.push_back(s.kfs[e[2]].mvInvLevelSigma2[kp.octave]);
  }
  x.eKF.push_back(2); x.eMP.push_back(3); x.eRight.push_back(0);   // point 5 <- keyframe 23, left
  x.eObs2.push_back(s.kfs[3].mvKeysUn[0].pt.x); x.eObs2.push_back(s.kfs[3].mvKeysUn[0].pt.y); x.eInv.push_back(s.kfs[3].mvInvLevelSigma2[0]);
}

int main() {
  {   // the flattening alone, host only
    Scene s;
    expect_of(s);
    WholeMapFlat<GBKeyFrame, GBMapPoint> f;
    morb_glue::flatten_whole_map(s.map.keyframes, s.map.points, f);
    const Expect& x = g_expect;
    REQUIRE(f.rig && f.kfs.size() == 4 && f.kfs[0] == &s.kfs[0] && f.kfs[1] == &s.kfs[2] && f.kfs[2] == &s.kfs[3] && f.kfs[3] == &s.kfs[4]);
    REQUIRE(f.mps.size() == 4 && f.mps[0] == &s.mps[0] && f.mps[1] == &s.mps[1] && f.mps[2] == &s.mps[4] && f.mps[3] == &s.mps[5]);
    REQUIRE(f.kfPose == x.kfPose && f.kfFixed == x.kfFixed && f.mpPos == x.mpPos && f.eKF == x.eKF && f.eMP == x.eMP && f.eRight == x.eRight && f.eInv == x.eInv);
    REQUIRE(f.eObs.size() == 3 * x.eKF.size());
    for (size_t e = 0; e < x.eKF.size(); ++e) REQUIRE(f.eObs[3 * e] == x.eObs2[2 * e] && f.eObs[3 * e + 1] == x.eObs2[2 * e + 1] && f.eObs[3 * e + 2] == -1.f);
  }
  {   // nLoopKF is the origin keyframe's id (20): SetPose / SetWorldPos / UpdateNormalAndDepth (:285-287, :354-356)
    Scene s;
    expect_of(s);
    g_calls = g_bad = 0;
    bool mbStopGBA = false;
    Optimizer::WholeMapBundleAdjustment(s.map.keyframes, s.map.points, 10, &mbStopGBA, 20, false);
    REQUIRE(g_calls == 1 && g_bad == 0 && g_its == 10 && g_robust == 0);
    for (int k = 0; k < 6; ++k) REQUIRE(s.kfs[k].nSetPose == ((k == 1 || k == 5) ? 0 : 1) && s.kfs[k].mnBAGlobalForKF == 0);
    REQUIRE(s.kfs[0].mTcw.q[3] == 0.99f && s.kfs[0].mTcw.t[2] == 2.f);                                  // the fixed keyframe: the pose it had
    REQUIRE(s.kfs[2].mTcw.q[0] == 107.f && s.kfs[2].mTcw.t[2] == 113.f && s.kfs[3].mTcw.q[0] == 114.f && s.kfs[4].mTcw.t[2] == 127.f);
    const int rows[4] = {0, 1, 4, 5};
    for (int r = 0; r < 4; ++r) {
      const GBMapPoint& p = s.mps[rows[r]];
      REQUIRE(p.nSetPos == 1 && p.nUpdates == 1 && p.mWorldPos.v[0] == 200.f + 3 * r && p.mWorldPos.v[2] == 202.f + 3 * r && p.mnBAGlobalForKF == 0);
    }
    for (int j : {2, 3, 6}) REQUIRE(s.mps[j].nSetPos == 0 && s.mps[j].nUpdates == 0);
  }
  {   // another nLoopKF, through GlobalBundleAdjustemnt with LoopClosing's five arguments: mTcwGBA / mPosGBA / mnBAGlobalForKF (:289-291, :358-359)
    Scene s;
    expect_of(s);
    g_calls = g_bad = 0;
    GBMap* pActiveMap = &s.map;
    bool mbStopGBA = false;
    const unsigned long nLoopKF = 23;
    Optimizer::GlobalBundleAdjustemnt(pActiveMap, 10, &mbStopGBA, nLoopKF, false);
    REQUIRE(g_calls == 1 && g_bad == 0 && g_its == 10 && g_robust == 0);
    for (int k = 0; k < 6; ++k) REQUIRE(s.kfs[k].nSetPose == 0 && s.kfs[k].mnBAGlobalForKF == ((k == 1 || k == 5) ? 0u : 23u));
    REQUIRE(s.kfs[2].mTcwGBA.q[0] == 107.f && s.kfs[2].mTcwGBA.t[2] == 113.f && s.kfs[0].mTcwGBA.q[3] == 0.99f && s.kfs[2].mTcw.q[3] == 0.99f);
    const int rows[4] = {0, 1, 4, 5};
    for (int r = 0; r < 4; ++r) {
      const GBMapPoint& p = s.mps[rows[r]];
      REQUIRE(p.nSetPos == 0 && p.nUpdates == 0 && p.mPosGBA.v[0] == 200.f + 3 * r && p.mnBAGlobalForKF == 23);
    }
    for (int j : {2, 3, 6}) REQUIRE(s.mps[j].mnBAGlobalForKF == 0);
  }
  std::printf("global ba member ok\n");
  return 0;
}
