// The reference-typed Optimizer::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag) of include/morb/Optimizer_reference.h on a
// mock map (tests/native/mock_merge_ba), with the call expression of LoopClosing::MergeLocal (src/LoopClosing.cc:1652-1653) unedited.
// Host side only: the few C entries the member reaches are STUBS defined here — morb_merge_bundle_adjustment checks the flattened graph
// against the expectation built by hand below and returns canned results — so the program needs neither the library nor a GPU and runs
// under -fsanitize=address,undefined.  Checked: which keyframes and points enter (bad ones, another map's, a keyframe of neither window),
// which observations become edges (monocular / stereo, a slot the keyframe no longer holds), the marks, the erase list, the poses and
// points written back, and that a raised stop flag leaves everything but the marks alone.
#include <cstdio>
#include <cstring>
#include <vector>

#include "merge_ba_mock.h"
#include "Optimizer.h"

using namespace ORB_SLAM3;
std::mutex ORB_SLAM3::MapPoint::mGlobalMutex;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// ---- stubs of the C entries the member reaches ----
static int g_calls = 0, g_bad = 0;
struct Expect { std::vector<float> kfPose, mpPos, eObs, eInv; std::vector<uint8_t> kfFixed; std::vector<int> eKF, eMP; float cam[5]; } g_expect;
static std::vector<uint8_t> g_erase;
extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
int morb_optimizer_create(morb_optimizer** out, int) { static int token; *out = reinterpret_cast<morb_optimizer*>(&token); return MORB_OK; }
int morb_optimizer_set_exact_order(morb_optimizer*, int) { return MORB_OK; }
const char* morb_last_error(void) { return "stub"; }
int morb_merge_bundle_adjustment(morb_optimizer*, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos, int nE, const int* eKF,
                                 const int* eMP, const float* eObs, const float* eInvSigma2, float fx, float fy, float cx, float cy, float bf,
                                 const uint8_t* stopFlag, uint8_t* eraseFlag, uint8_t* levelFlag, int* stats6) {
  ++g_calls;
  const Expect& x = g_expect;
  auto same = [](const auto& v, const auto* p, size_t n) { return v.size() == n && (n == 0 || std::memcmp(v.data(), p, n * sizeof(v[0])) == 0); };
  if (!same(x.kfPose, kfPose, (size_t)nKF * 7) || !same(x.kfFixed, kfFixed, nKF) || !same(x.mpPos, mpPos, (size_t)nMP * 3) || !same(x.eKF, eKF, nE) ||
      !same(x.eMP, eMP, nE) || !same(x.eObs, eObs, (size_t)nE * 3) || !same(x.eInv, eInvSigma2, nE) || fx != x.cam[0] || fy != x.cam[1] ||
      cx != x.cam[2] || cy != x.cam[3] || bf != x.cam[4] || !stopFlag || *stopFlag)
    ++g_bad;
  for (int i = 0; i < nKF * 7; ++i) kfPose[i] = 100.f + i;      // (fixed keyframes too: the member must not write them back)
  for (int i = 0; i < nMP * 3; ++i) mpPos[i] = 200.f + i;
  for (int e = 0; e < nE; ++e) { eraseFlag[e] = e < (int)g_erase.size() ? g_erase[e] : 0; levelFlag[e] = eraseFlag[e]; }
  const int s[6] = {5, 5, 7, 7, 1, 2};
  std::memcpy(stats6, s, sizeof s);
  return MORB_OK;
}
int morb_merge_bundle_adjustment_fisheye(morb_optimizer*, int, float*, const uint8_t*, int, float*, int, const int*, const int*, const float*, const float*,
                                         const float*, const uint8_t*, uint8_t*, uint8_t*, int*) { ++g_bad; return MORB_ERR_INVALID; }
}

struct Scene {
  MBMap map, other;
  GeometricCamera cam;
  std::vector<MBKeyFrame> kfs;
  std::vector<MBMapPoint> mps;
  Scene() : kfs(6), mps(6) {
    cam.mvParameters = {458.f, 457.f, 367.f, 248.f};
    for (int k = 0; k < 6; ++k) {
      MBKeyFrame& K = kfs[k];
      K.mnId = 10 + k; K.mpMap = &map; K.mpCamera = &cam; K.fx = 458.f; K.fy = 457.f; K.cx = 367.f; K.cy = 248.f; K.mbf = 50.f;
      K.mvInvLevelSigma2 = {1.f, 0.5f, 0.25f};
      K.N = 8; K.mvKeysUn.resize(8); K.mvuRight.assign(8, -1.f); K.mvpMapPoints.assign(8, nullptr);
      for (int i = 0; i < 8; ++i) { K.mvKeysUn[i].pt.x = 100.f * k + i; K.mvKeysUn[i].pt.y = 50.f * k + 2 * i; K.mvKeysUn[i].octave = i % 3; }
      const float q[4] = {0.01f * k, 0.02f, 0.03f, 0.99f};
      for (int c = 0; c < 4; ++c) K.mTcw.q[c] = q[c];
      for (int c = 0; c < 3; ++c) K.mTcw.t[c] = 0.5f * k + c;
    }
    kfs[2].mbBad = true;        // a bad keyframe of the free window
    kfs[4].mpMap = &other;      // a keyframe of the fixed window that is in another map
    for (int j = 0; j < 6; ++j) { mps[j].mnId = j; mps[j].mpMap = &map; mps[j].mWorldPos = Eigen::Vector3f(1.f + j, 2.f + j, 5.f + j); }
    mps[2].mbBad = true;        // a bad point
    mps[3].mpMap = &other;      // a point of another map
    auto see = [&](int k, int j, int idx, float ur = -1.f) { kfs[k].mvpMapPoints[idx] = &mps[j]; kfs[k].mvuRight[idx] = ur; mps[j].AddObservation(&kfs[k], idx, -1); };
    see(0, 0, 1); see(1, 0, 2); see(3, 0, 3);                    // point 0: two free keyframes and the fixed one, monocular
    see(0, 1, 4); see(3, 1, 5, 77.5f); see(5, 1, 0);             // point 1: stereo in the fixed keyframe; keyframe 5 is in neither window
    see(0, 2, 6); see(1, 3, 6);                                  // the bad point, the other map's point
    see(0, 4, 7); see(1, 4, 7); kfs[1].mvpMapPoints[7] = nullptr;   // point 4: keyframe 1 no longer holds it at that index
    see(2, 5, 0); see(4, 5, 0);                                  // point 5: only seen by the keyframes that do not enter
    mps[1].AddObservation(&kfs[2], 3, -1);                       // ... and an observation by the bad keyframe
  }
};

int main() {
  // vertices: the fixed window first (keyframe 3), then the free one (0, 1); points in the order the keyframes' sets give them: 0, 1 (keyframe 3),
  // 4 (keyframe 0).  Edges by point, observations by keyframe address: point 0 <- 0, 1, 3; point 1 <- 0, 3 (stereo); point 4 <- 0.
  {
    Scene s;
    Expect& x = g_expect;
    x = Expect();
    for (int k : {3, 0, 1}) { for (int c = 0; c < 4; ++c) x.kfPose.push_back(s.kfs[k].mTcw.q[c]); for (int c = 0; c < 3; ++c) x.kfPose.push_back(s.kfs[k].mTcw.t[c]); }
    x.kfFixed = {1, 0, 0};
    for (int j : {0, 1, 4}) for (int c = 0; c < 3; ++c) x.mpPos.push_back(s.mps[j].mWorldPos(c));
    const int edges[6][4] = {{1, 0, 0, 1}, {2, 0, 1, 2}, {0, 0, 3, 3}, {1, 1, 0, 4}, {0, 1, 3, 5}, {1, 2, 0, 7}};   // vertex, point, keyframe, keypoint
    for (const auto& e : edges) {
      x.eKF.push_back(e[0]); x.eMP.push_back(e[1]);
      const cv::KeyPoint& kp = s.kfs[e[2]].mvKeysUn[e[3]];
      x.eObs.push_back(kp.pt.x); x.eObs.push_back(kp.pt.y); x.eObs.push_back(s.kfs[e[2]].mvuRight[e[3]] < 0 ? -1.f : s.kfs[e[2]].mvuRight[e[3]]);
      x.eInv.push_back(s.kfs[e[2]].mvInvLevelSigma2[kp.octave]);
    }
    const float cam[5] = {458.f, 457.f, 367.f, 248.f, 50.f};
    std::memcpy(x.cam, cam, sizeof cam);
    g_erase = {0, 1, 0, 0, 1, 0};   // erase (keyframe 1, point 0) and (keyframe 3, point 1)
    g_calls = g_bad = 0;
    MBKeyFrame* mpCurrentKF = &s.kfs[0];
    std::vector<MBKeyFrame*> vpLocalCurrentWindowKFs = {&s.kfs[0], &s.kfs[1], &s.kfs[2]}, vpMergeConnectedKFs = {&s.kfs[3], &s.kfs[4]};
    bool bStop = false;
    // src/LoopClosing.cc:1652-1653, unedited
    Optimizer::LocalBundleAdjustment(mpCurrentKF, vpLocalCurrentWindowKFs,
                                     vpMergeConnectedKFs, &bStop);
    REQUIRE(g_calls == 1 && g_bad == 0);
    const long unsigned int id = s.kfs[0].mnId;
    for (int k = 0; k < 6; ++k) REQUIRE(s.kfs[k].mnBALocalForMerge == ((k == 0 || k == 1 || k == 3) ? id : 0));
    for (int j = 0; j < 6; ++j) REQUIRE(s.mps[j].mnBALocalForMerge == ((j == 0 || j == 1 || j == 4) ? id : 0));
    // poses: vertices 1 and 2 (keyframes 0 and 1) written from the entry's output, the fixed and the outside keyframes untouched
    for (int k = 0; k < 6; ++k) REQUIRE(s.kfs[k].nSetPose == ((k == 0 || k == 1) ? 1 : 0));
    REQUIRE(s.kfs[0].mTcw.q[0] == 107.f && s.kfs[0].mTcw.q[3] == 110.f && s.kfs[0].mTcw.t[2] == 113.f);
    REQUIRE(s.kfs[1].mTcw.q[0] == 114.f && s.kfs[1].mTcw.t[0] == 118.f);
    // points 0, 1, 4 <- rows 0, 1, 2
    const int rows[3] = {0, 1, 4};
    for (int r = 0; r < 3; ++r) {
      const MBMapPoint& p = s.mps[rows[r]];
      REQUIRE(p.nSetPos == 1 && p.nUpdates == 1 && p.mWorldPos.v[0] == 200.f + 3 * r && p.mWorldPos.v[2] == 202.f + 3 * r);
    }
    for (int j : {2, 3, 5}) REQUIRE(s.mps[j].nSetPos == 0 && s.mps[j].nUpdates == 0);
    // erased: both sides of the two observations, nothing else
    REQUIRE(s.kfs[1].mvpMapPoints[2] == nullptr && s.mps[0].mObservations.count(&s.kfs[1]) == 0);
    REQUIRE(s.kfs[3].mvpMapPoints[5] == nullptr && s.mps[1].mObservations.count(&s.kfs[3]) == 0);
    REQUIRE(s.kfs[0].mvpMapPoints[1] == &s.mps[0] && s.kfs[3].mvpMapPoints[3] == &s.mps[0] && s.kfs[0].mvpMapPoints[4] == &s.mps[1]);
    REQUIRE(s.mps[0].mObservations.size() == 2 && s.mps[1].mObservations.size() == 3 && s.kfs[0].mvpMapPoints[7] == &s.mps[4]);
  }
  {   // *pbStopFlag set: the graph is selected and marked, nothing reaches the device, nothing is written (:3650-3651)
    Scene s;
    g_calls = g_bad = 0;
    bool bStop = true;
    Optimizer::LocalBundleAdjustment(&s.kfs[0], std::vector<MBKeyFrame*>{&s.kfs[0], &s.kfs[1]}, std::vector<MBKeyFrame*>{&s.kfs[3]}, &bStop);
    REQUIRE(g_calls == 0);
    REQUIRE(s.kfs[0].mnBALocalForMerge == s.kfs[0].mnId && s.kfs[3].mnBALocalForMerge == s.kfs[0].mnId && s.mps[0].mnBALocalForMerge == s.kfs[0].mnId);
    for (int k = 0; k < 6; ++k) REQUIRE(s.kfs[k].nSetPose == 0);
    for (int j = 0; j < 6; ++j) REQUIRE(s.mps[j].nSetPos == 0 && s.mps[j].nUpdates == 0);
  }
  {   // windows whose keyframes are all bad or foreign: an empty graph, no call
    Scene s;
    g_calls = 0;
    bool bStop = false;
    Optimizer::LocalBundleAdjustment(&s.kfs[0], std::vector<MBKeyFrame*>{&s.kfs[2]}, std::vector<MBKeyFrame*>{&s.kfs[4]}, &bStop);
    REQUIRE(g_calls == 0 && s.kfs[2].mnBALocalForMerge == 0 && s.kfs[4].mnBALocalForMerge == 0);
  }
  std::printf("merge ba member ok\n");
  return 0;
}
