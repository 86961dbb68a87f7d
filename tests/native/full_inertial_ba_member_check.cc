// The reference-typed Optimizer::FullInertialBA(pMap, its, bFixLocal, nLoopId, pbStopFlag, bInit, priorG, priorA) of
// include/morb/Optimizer_reference.h on a mock map (tests/native/mock_full_inertial_ba), with the call expressions of
// LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:2305) and LocalMapping::InitializeIMU (src/LocalMapping.cc:1244-1249) unedited.
// Host side only: the C entries the member reaches are STUBS defined here — they check the flattened graph against the expectation built by
// hand below and return canned results — so the program needs neither the library nor a GPU and runs under -fsanitize=address,undefined.
// Checked: the vertices by ascending mnId, a bad keyframe, a keyframe without IMU, a keyframe beyond maxKFid, a missing mPrevKF, the kinds,
// the links and SetNewBias on their preintegrations, which observations become edges, a point nobody usable sees, a rig keyframe with left
// and right observations, bFixLocal with 2 and with 3 free keyframes, both write-backs, the shared-bias write-back, the handle per caller and a
// raised stop flag.
#include <cstdio>
#include <cstring>
#include <vector>

#include "full_inertial_ba_mock.h"
#include "Optimizer.h"

using namespace ORB_SLAM3;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// ---- stubs of the C entries the member reaches ----
static int g_calls = 0, g_bad = 0, g_creates = 0, g_fisheye = 0;
struct Expect {
  std::vector<float> kfState, mpPos, eObs, eInv, preDT;
  std::vector<uint8_t> kfKind, eRight;
  std::vector<int> eKF, eMP, iKF1, iKF2;
  int its = 0, bInit = 0; float priorG = 0, priorA = 0, bias6[6] = {0, 0, 0, 0, 0, 0}; bool stop = false;
} g_expect;
static int stub(int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos, int nE, const int* eKF, const int* eMP, const float* eObs,
                const uint8_t* eRight, const float* eInvSigma2, int nI, const int* iKF1, const int* iKF2, const morb_imu_preintegrated* iPre,
                const float* Tbc12, int its, int bInit, float priorG, float priorA, float* bias6, const uint8_t* pbStopFlag, int* stats4, double* chi2) {
  ++g_calls;
  const Expect& x = g_expect;
  auto same = [](const auto& v, const auto* p, size_t n) { return v.size() == n && (n == 0 || std::memcmp(v.data(), p, n * sizeof(v[0])) == 0); };
  if (!same(x.kfState, kfState21, (size_t)nKF * 21) || !same(x.kfKind, kfKind, nKF) || !same(x.mpPos, mpPos, (size_t)nMP * 3) || !same(x.eKF, eKF, nE) ||
      !same(x.eMP, eMP, nE) || !same(x.eObs, eObs, (size_t)nE * 3) || !same(x.eInv, eInvSigma2, nE) || !same(x.iKF1, iKF1, nI) || !same(x.iKF2, iKF2, nI) ||
      (eRight && !same(x.eRight, eRight, nE)) || its != x.its || bInit != x.bInit || priorG != x.priorG || priorA != x.priorA ||
      (pbStopFlag != nullptr) != x.stop || (pbStopFlag && *pbStopFlag) || std::memcmp(bias6, x.bias6, sizeof x.bias6) != 0)
    ++g_bad;
  for (int i = 0; i < nI && i < (int)x.preDT.size(); ++i) if (iPre[i].dT != x.preDT[i]) ++g_bad;
  const float I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  if (std::memcmp(Tbc12, I, sizeof I) != 0) ++g_bad;
  for (int k = 0; k < nKF; ++k) {   // as the entry writes: kind 0 everything, kind 3 the pose, kinds 1 and 2 nothing; Rwb = I, the rest numbered
    float* s = kfState21 + 21 * k;
    if (kfKind[k] == 1 || kfKind[k] == 2) continue;
    for (int i = 0; i < 9; ++i) s[i] = I[i];
    for (int i = 9; i < (kfKind[k] == 0 ? 21 : 12); ++i) s[i] = 100.f + 21 * k + i;
  }
  for (int i = 0; i < nMP * 3; ++i) mpPos[i] = 200.f + i;
  if (bInit) for (int k = 0; k < 6; ++k) bias6[k] = 9.f - k;
  stats4[0] = 3; stats4[1] = 4; stats4[2] = 15; stats4[3] = 15; chi2[0] = 2; chi2[1] = 1;
  return MORB_OK;
}
extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
int morb_optimizer_create(morb_optimizer** out, int) { static int token[8]; *out = reinterpret_cast<morb_optimizer*>(&token[g_creates++ & 7]); return MORB_OK; }
int morb_optimizer_set_exact_order(morb_optimizer*, int) { return MORB_OK; }
const char* morb_last_error(void) { return "stub"; }
int morb_full_inertial_ba(morb_optimizer*, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos, int nE, const int* eKF, const int* eMP,
                          const float* eObs, const float* eInvSigma2, int nI, const int* iKF1, const int* iKF2, const morb_imu_preintegrated* iPre, float fx,
                          float fy, float cx, float cy, float bf, const float* Tbc12, int its, int bInit, float priorG, float priorA, float* bias6,
                          const uint8_t* pbStopFlag, int* stats4, double* chi2) {
  if (fx != 458.f || fy != 457.f || cx != 367.f || cy != 248.f || bf != 50.f) ++g_bad;
  return stub(nKF, kfState21, kfKind, nMP, mpPos, nE, eKF, eMP, eObs, nullptr, eInvSigma2, nI, iKF1, iKF2, iPre, Tbc12, its, bInit, priorG, priorA, bias6,
              pbStopFlag, stats4, chi2);
}
int morb_full_inertial_ba_fisheye(morb_optimizer*, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos, int nE, const int* eKF,
                                  const int* eMP, const float* eObs, const uint8_t* eRight, const float* eInvSigma2, int nI, const int* iKF1, const int* iKF2,
                                  const morb_imu_preintegrated* iPre, const float* rig28, const float* Tbc12, int its, int bInit, float priorG, float priorA,
                                  float* bias6, const uint8_t* pbStopFlag, int* stats4, double* chi2) {
  ++g_fisheye;
  if (!eRight || rig28[0] != 190.f || rig28[8] != 191.f || rig28[25] != -0.1f) ++g_bad;
  return stub(nKF, kfState21, kfKind, nMP, mpPos, nE, eKF, eMP, eObs, eRight, eInvSigma2, nI, iKF1, iKF2, iPre, Tbc12, its, bInit, priorG, priorA, bias6,
              pbStopFlag, stats4, chi2);
}
}

// Six keyframes with ids 0 .. 5 in one chain K0 <- K1 <- K2 <- K3 <- K4 <- K5, handed over as K2, K0, K1, K4, K3, K5.  K3 is bad, K4 has no IMU,
// K5 lies beyond maxKFid = 4, K0 has no mPrevKF.  Points: 0 seen by K0 (mono), K1 (stereo), K3 (bad: skipped), K5 (beyond: skipped); 1 by K4;
// 2 by nobody; 3 by K5 alone.
enum { K0, K1, K2, K3, K4, K5, NKF };
struct Scene {
  FIMap map;
  FIAtlas atlas;
  GeometricCamera camL, camR;
  std::vector<FIKeyFrame> kfs;
  std::vector<FIMapPoint> mps;
  std::vector<FIPreintegrated> pre;
  explicit Scene(bool rig = false) : kfs(NKF), mps(4), pre(NKF) {
    camL.mvParameters = {190.f, 190.f, 254.f, 256.f, 0.1f, 0.2f, 0.3f, 0.4f}; camR.mvParameters = {191.f, 191.f, 252.f, 255.f, 0.5f, 0.6f, 0.7f, 0.8f};
    for (int k = 0; k < NKF; ++k) {
      FIKeyFrame& K = kfs[k];
      K.mnId = k; K.fx = 458.f; K.fy = 457.f; K.cx = 367.f; K.cy = 248.f; K.mbf = 50.f;
      K.mvInvLevelSigma2 = {1.f, 0.5f, 0.25f};
      K.mvKeysUn.resize(4); K.mvuRight.assign(4, -1.f);
      for (int i = 0; i < 4; ++i) { K.mvKeysUn[i].pt.x = 100.f * k + i; K.mvKeysUn[i].pt.y = 50.f * k + 2 * i; K.mvKeysUn[i].octave = (i + k) % 3; }
      for (int c = 0; c < 3; ++c) { K.mOwb(c) = 0.5f * k + c; K.mVw(c) = 0.1f * k + c; }
      K.mRwb(0, 1) = 0.01f * k;
      K.mImuBias = IMU::Bias(0.1f + k, 0.2f + k, 0.3f + k, 0.4f + k, 0.5f + k, 0.6f + k);
      pre[k].dT = 1.f + k;
      if (k) { K.mPrevKF = &kfs[k - 1]; K.mpImuPreintegrated = &pre[k]; }
      if (rig) {
        K.mpCamera = &camL; K.mpCamera2 = &camR; K.NLeft = 4; K.mvKeysRight.resize(8); K.mTrl.t[0] = -0.1f;
        for (int i = 0; i < 8; ++i) { K.mvKeysRight[i].pt.x = 1000.f + 100.f * k + i; K.mvKeysRight[i].pt.y = 2000.f + 50.f * k + i; K.mvKeysRight[i].octave = (i + 1) % 3; }
      }
    }
    kfs[K3].mbBad = true; kfs[K4].bImu = false;
    for (int j = 0; j < 4; ++j) { mps[j].mnId = j; mps[j].mWorldPos = Eigen::Vector3f(1.f + j, 2.f + j, 5.f + j); map.mps.push_back(&mps[j]); }
    for (int k : {K2, K0, K1, K4, K3, K5}) map.kfs.push_back(&kfs[k]);
    map.maxKFid = 4;
    atlas.current = &map;
    see(K0, 0, 0); see(K1, 0, 1, rig ? -1.f : 77.5f, rig ? 5 : -1); see(K3, 0, 2); see(K5, 0, 3);
    see(K4, 1, 2);
    see(K5, 3, 0);
    if (rig) mps[1].mObservations[&kfs[K2]] = std::make_tuple(-1, 6);      // the right camera alone
  }
  void see(int k, int j, int idx, float ur = -1.f, int right = -1) { kfs[k].mvuRight[idx] = ur; mps[j].mObservations[&kfs[k]] = std::make_tuple(idx, right); }
};
struct Link { int r1, r2, kf; };
struct Edge { int row, pt, kf, kp, right; };
static void expect(Scene& s, const std::vector<uint8_t>& kinds, const std::vector<Link>& links, const std::vector<Edge>& edges, int its, int bInit, float pG,
                   float pA, bool stop) {
  Expect& x = g_expect;
  x = Expect();
  for (int k = 0; k < 5; ++k) {   // vertices: ids 0 .. 4 in ascending order
    const FIKeyFrame& K = s.kfs[k];
    for (int i = 0; i < 9; ++i) x.kfState.push_back(K.mRwb.m[i]);
    for (int c = 0; c < 3; ++c) x.kfState.push_back(K.mOwb.v[c]);
    for (int c = 0; c < 3; ++c) x.kfState.push_back(K.mVw.v[c]);
    const IMU::Bias& b = K.mImuBias;
    for (float v : {b.bwx, b.bwy, b.bwz, b.bax, b.bay, b.baz}) x.kfState.push_back(v);
  }
  x.kfKind = kinds;
  for (int j = 0; j < 4; ++j) for (int c = 0; c < 3; ++c) x.mpPos.push_back(s.mps[j].mWorldPos(c));
  for (const Link& l : links) { x.iKF1.push_back(l.r1); x.iKF2.push_back(l.r2); x.preDT.push_back(s.pre[l.kf].dT); }
  for (const Edge& e : edges) {
    x.eKF.push_back(e.row); x.eMP.push_back(e.pt); x.eRight.push_back((uint8_t)e.right);
    const cv::KeyPoint& kp = e.right ? s.kfs[e.kf].mvKeysRight[e.kp] : s.kfs[e.kf].mvKeysUn[e.kp];
    x.eObs.push_back(kp.pt.x); x.eObs.push_back(kp.pt.y); x.eObs.push_back(e.right || s.kfs[e.kf].mvuRight[e.kp] < 0 ? -1.f : s.kfs[e.kf].mvuRight[e.kp]);
    x.eInv.push_back(s.kfs[e.kf].mvInvLevelSigma2[kp.octave]);
  }
  x.its = its; x.bInit = bInit; x.priorG = pG; x.priorA = pA; x.stop = stop;
  const IMU::Bias& b = s.kfs[K3].mImuBias;   // pIncKF: the last keyframe of GetAllKeyFrames() within maxKFid
  const float b6[6] = {b.bwx, b.bwy, b.bwz, b.bax, b.bay, b.baz};
  std::memcpy(x.bias6, b6, sizeof b6);
}

int main() {
  // links in the order of GetAllKeyFrames(): K2 (K1 -> K2), K1 (K0 -> K1); K4 has no IMU, K3 is bad, K5 is beyond maxKFid
  const std::vector<Link> links = {{1, 2, K2}, {0, 1, K1}};
  const std::vector<Edge> edges = {{0, 0, K0, 0, 0}, {1, 0, K1, 1, 0}, {4, 1, K4, 2, 0}};
  {   // LoopClosing: a loop id, the stop flag, the loop-closing handle; the GBA members are written
    Scene s;
    expect(s, {0, 0, 0, 3, 3}, links, edges, 7, 0, 1e2f, 1e6f, true);
    g_calls = g_bad = 0;
    FIMap* pActiveMap = &s.map;
    const unsigned long nLoopKF = 7;
    bool mbStopGBA = false;
    // src/LoopClosing.cc:2305, unedited
    Optimizer::FullInertialBA(pActiveMap, 7, false, nLoopKF, &mbStopGBA);
    REQUIRE(g_calls == 1 && g_bad == 0 && g_fisheye == 0);
    for (int k : {K1, K2}) REQUIRE(s.pre[k].nSetNewBias == 1 && s.pre[k].last.bax == 0.1f + (k - 1));
    REQUIRE(s.pre[K4].nSetNewBias == 0 && s.pre[K5].nSetNewBias == 0 && s.pre[K3].nSetNewBias == 0);   // (K4 -> K5: K5 is beyond maxKFid; K3 is bad)
    for (int k = 0; k < 5; ++k) {
      FIKeyFrame& K = s.kfs[k];
      REQUIRE(K.mnBAGlobalForKF == 7 && K.nSetPose == 0 && K.nSetVelocity == 0 && K.nSetNewBias == 0);
      for (int c = 0; c < 3; ++c) REQUIRE(K.mTcwGBA.t[c] == -(100.f + 21 * k + 9 + c));   // (Tbc = I, Rwb = I: tcw = -twb)
      if (k <= K2) REQUIRE(K.mVwbGBA(0) == 100.f + 21 * k + 12 && K.mBiasGBA.bwx == 100.f + 21 * k + 15 && K.mBiasGBA.baz == 100.f + 21 * k + 20);
      if (k == K3) REQUIRE(K.mVwbGBA(0) == K.mVw(0) && K.mBiasGBA.bax == K.mImuBias.bax);      // (bImu without a link: its own velocity and bias)
    }
    REQUIRE(s.kfs[K4].mVwbGBA(1) == 0.f && s.kfs[K5].mnBAGlobalForKF == 0);
    for (int j : {0, 1}) REQUIRE(s.mps[j].mnBAGlobalForKF == 7 && s.mps[j].mPosGBA.v[0] == 200.f + 3 * j && s.mps[j].nSetPos == 0);
    for (int j : {2, 3}) REQUIRE(s.mps[j].mnBAGlobalForKF == 0);
    REQUIRE(s.map.changes == 1 && g_creates == 1);
  }
  {   // LocalMapping with the priors: bInit, no stop flag, the mapping handle; nLoopId is the keyframe's id, 0 here: the map itself is written
    Scene s;
    expect(s, {0, 0, 0, 3, 3}, links, edges, 100, 1, 1e2f, 1e10f, false);
    g_calls = g_bad = 0;
    FIAtlas* mpAtlas = &s.atlas;
    FIKeyFrame* mpCurrentKeyFrame = &s.kfs[K0];
    const float priorG = 1e2f, priorA = 1e10f;
    // src/LocalMapping.cc:1244-1246, unedited
    Optimizer::FullInertialBA(mpAtlas->GetCurrentMap(), 100, false,
                              mpCurrentKeyFrame->mnId, NULL, true, priorG,
                              priorA);
    REQUIRE(g_calls == 1 && g_bad == 0 && g_creates == 2);
    for (int k = 0; k < 5; ++k) {
      FIKeyFrame& K = s.kfs[k];
      REQUIRE(K.nSetPose == 1 && K.mnBAGlobalForKF == 0 && K.nSetVelocity == (k == K4 ? 0 : 1) && K.nSetNewBias == (k == K4 ? 0 : 1));
      if (k != K4) REQUIRE(K.mImuBias.bwx == 9.f && K.mImuBias.bwz == 7.f && K.mImuBias.bax == 6.f && K.mImuBias.baz == 4.f);   // the shared bias, every bImu keyframe
    }
    REQUIRE(s.kfs[K1].mVw(0) == 100.f + 21 * K1 + 12 && s.kfs[K3].mVw(0) == 0.1f * K3);
    for (int j : {0, 1}) REQUIRE(s.mps[j].nSetPos == 1 && s.mps[j].nUpdates == 1 && s.mps[j].mWorldPos.v[2] == 202.f + 3 * j);
    REQUIRE(s.mps[2].nSetPos == 0 && s.mps[3].nSetPos == 0 && s.map.changes == 1);
  }
  {   // LocalMapping without the priors, on a KannalaBrandt8 rig: left and right observations, the right camera alone
    Scene s(true);
    expect(s, {0, 0, 0, 3, 3}, links, {{0, 0, K0, 0, 0}, {1, 0, K1, 1, 0}, {1, 0, K1, 1, 1}, {2, 1, K2, 2, 1}, {4, 1, K4, 2, 0}}, 100, 0, 1e2f, 1e6f, false);
    g_calls = g_bad = 0;
    FIAtlas* mpAtlas = &s.atlas;
    FIKeyFrame* mpCurrentKeyFrame = &s.kfs[K0];
    // src/LocalMapping.cc:1248-1249, unedited
    Optimizer::FullInertialBA(mpAtlas->GetCurrentMap(), 100, false,
                              mpCurrentKeyFrame->mnId, NULL, false);
    REQUIRE(g_calls == 1 && g_bad == 0 && g_fisheye == 1 && g_creates == 2);
    REQUIRE(s.kfs[K2].mImuBias.bwx == 100.f + 21 * K2 + 15 && s.kfs[K3].mImuBias.bwx == 0.4f + K3 && s.kfs[K2].nSetPose == 1);
  }
  {   // bFixLocal: K3 and K4 carry the local-BA marks of the newest keyframes -> fixed; three keyframes stay free
    Scene s;
    s.kfs[K3].mnBALocalForKF = 4; s.kfs[K4].mnBAFixedForKF = 3;
    expect(s, {0, 0, 0, 2, 2}, links, {{0, 0, K0, 0, 0}, {1, 0, K1, 1, 0}}, 5, 0, 1e2f, 1e6f, false);   // point 1 is seen by a fixed keyframe alone: no edge
    g_calls = g_bad = 0;
    Optimizer::FullInertialBA(&s.map, 5, true);
    REQUIRE(g_calls == 1 && g_bad == 0);
    REQUIRE(s.mps[0].nSetPos == 1 && s.mps[1].nSetPos == 0);
    REQUIRE(s.kfs[K4].mTcw.t[0] == -s.kfs[K4].mOwb(0) && s.kfs[K4].nSetPose == 1);   // (a fixed keyframe is written with the pose it has)
    Scene t;   // two free keyframes: nothing happens at all (:438-440)
    t.kfs[K3].mnBALocalForKF = 4; t.kfs[K4].mnBAFixedForKF = 3; t.kfs[K2].mnBALocalForKF = 3;
    g_calls = 0;
    Optimizer::FullInertialBA(&t.map, 5, true);
    REQUIRE(g_calls == 0 && t.map.changes == 0 && t.pre[K1].nSetNewBias == 0 && t.kfs[K0].nSetPose == 0);
  }
  {   // *pbStopFlag set: the preintegrations take their bias, nothing reaches the device, nothing is written (:689)
    Scene s;
    g_calls = 0;
    bool bStop = true;
    Optimizer::FullInertialBA(&s.map, 7, false, 7, &bStop);
    REQUIRE(g_calls == 0 && s.map.changes == 0 && s.pre[K1].nSetNewBias == 1 && s.kfs[K0].mnBAGlobalForKF == 0 && s.mps[0].mnBAGlobalForKF == 0);
  }
  std::printf("full inertial ba member ok\n");
  return 0;
}
