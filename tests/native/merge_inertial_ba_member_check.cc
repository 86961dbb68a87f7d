// The reference-typed Optimizer::MergeInertialBA(pCurrKF, pMergeKF, pbStopFlag, pMap, corrPoses) of include/morb/Optimizer_reference.h on a
// mock map (tests/native/mock_merge_inertial_ba), with the call expression of LoopClosing::MergeLocal (src/LoopClosing.cc:1649-1650)
// unedited.  Host side only: the few C entries the member reaches are STUBS defined here — morb_merge_inertial_ba checks the flattened graph
// against the expectation built by hand below and returns canned results — so the program needs neither the library nor a GPU and runs
// under -fsanitize=address,undefined.  Checked: the two windows and the covisible selection (the head of the current chain, a keyframe
// newer than the current one, a keyframe without IMU), the kinds, the links, which observations become edges, the marks, SetNewBias on
// the preintegrations, the erase list, poses / velocities / biases / corrPoses / points written back, and a raised stop flag.
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "merge_inertial_ba_mock.h"
#include "Optimizer.h"

using namespace ORB_SLAM3;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// ---- stubs of the C entries the member reaches ----
static int g_calls = 0, g_bad = 0;
struct Expect { std::vector<float> kfState, mpPos, eObs, eInv; std::vector<uint8_t> kfKind; std::vector<int> eKF, eMP, iKF1, iKF2; std::vector<float> preDT; float cam[5]; } g_expect;
static std::vector<uint8_t> g_erase;
extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
int morb_optimizer_create(morb_optimizer** out, int) { static int token; *out = reinterpret_cast<morb_optimizer*>(&token); return MORB_OK; }
int morb_optimizer_set_exact_order(morb_optimizer*, int) { return MORB_OK; }
const char* morb_last_error(void) { return "stub"; }
int morb_merge_inertial_ba(morb_optimizer*, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos, int nE, const int* eKF, const int* eMP,
                           const float* eObs, const float* eInvSigma2, int nI, const int* iKF1, const int* iKF2, const morb_imu_preintegrated* iPre, float fx,
                           float fy, float cx, float cy, float bf, const float* Tbc12, const uint8_t* pbStopFlag, uint8_t* eraseFlag, int* stats3) {
  ++g_calls;
  const Expect& x = g_expect;
  auto same = [](const auto& v, const auto* p, size_t n) { return v.size() == n && (n == 0 || std::memcmp(v.data(), p, n * sizeof(v[0])) == 0); };
  if (!same(x.kfState, kfState21, (size_t)nKF * 21) || !same(x.kfKind, kfKind, nKF) || !same(x.mpPos, mpPos, (size_t)nMP * 3) || !same(x.eKF, eKF, nE) ||
      !same(x.eMP, eMP, nE) || !same(x.eObs, eObs, (size_t)nE * 3) || !same(x.eInv, eInvSigma2, nE) || !same(x.iKF1, iKF1, nI) || !same(x.iKF2, iKF2, nI) ||
      fx != x.cam[0] || fy != x.cam[1] || cx != x.cam[2] || cy != x.cam[3] || bf != x.cam[4] || !pbStopFlag || *pbStopFlag)
    ++g_bad;
  for (int i = 0; i < nI && i < (int)x.preDT.size(); ++i) if (iPre[i].dT != x.preDT[i]) ++g_bad;
  const float I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  if (std::memcmp(Tbc12, I, sizeof I) != 0) ++g_bad;
  for (int k = 0; k < nKF; ++k) {   // (every row, fixed ones too: the member must not write those back) Rwb = I, the rest numbered
    float* s = kfState21 + 21 * k;
    for (int i = 0; i < 9; ++i) s[i] = I[i];
    for (int i = 9; i < 21; ++i) s[i] = 100.f + 21 * k + i;
  }
  for (int i = 0; i < nMP * 3; ++i) mpPos[i] = 200.f + i;
  for (int e = 0; e < nE; ++e) eraseFlag[e] = e < (int)g_erase.size() ? g_erase[e] : 0;
  stats3[0] = 8; stats3[1] = 9; stats3[2] = 1;
  return MORB_OK;
}
int morb_merge_inertial_ba_fisheye(morb_optimizer*, int, float*, const uint8_t*, int, float*, int, const int*, const int*, const float*, const float*, int,
                                   const int*, const int*, const morb_imu_preintegrated*, const float*, const float*, const uint8_t*, uint8_t*, int*) {
  ++g_bad; return MORB_ERR_INVALID;
}
}

enum { A0, A1, A2, B0, B1, B2, B3, C0, D, NKF };
struct Scene {
  MIMap map;
  std::vector<MIKeyFrame> kfs;
  std::vector<MIMapPoint> mps;
  std::vector<MIPreintegrated> pre;
  Scene() : kfs(NKF), mps(4), pre(NKF) {
    const long unsigned int ids[NKF] = {20, 21, 22, 5, 6, 7, 8, 3, 30};   // D is newer than the current keyframe (A2)
    for (int k = 0; k < NKF; ++k) {
      MIKeyFrame& K = kfs[k];
      K.mnId = ids[k]; K.fx = 458.f; K.fy = 457.f; K.cx = 367.f; K.cy = 248.f; K.mbf = 50.f;
      K.mvInvLevelSigma2 = {1.f, 0.5f, 0.25f};
      K.mvKeysUn.resize(4); K.mvuRight.assign(4, -1.f); K.mvpMapPoints.assign(4, nullptr);
      for (int i = 0; i < 4; ++i) { K.mvKeysUn[i].pt.x = 100.f * k + i; K.mvKeysUn[i].pt.y = 50.f * k + 2 * i; K.mvKeysUn[i].octave = (i + k) % 3; }
      for (int c = 0; c < 3; ++c) { K.mOwb(c) = 0.5f * k + c; K.mVw(c) = 0.1f * k + c; }
      K.mRwb(0, 1) = 0.01f * k;
      K.mImuBias = IMU::Bias(0.1f + k, 0.2f + k, 0.3f + k, 0.4f + k, 0.5f + k, 0.6f + k);
      pre[k].dT = 1.f + k;
    }
    auto chain = [&](std::initializer_list<int> c) { int prev = -1; for (int k : c) { if (prev >= 0) { kfs[k].mPrevKF = &kfs[prev]; kfs[prev].mNextKF = &kfs[k]; kfs[k].mpImuPreintegrated = &pre[k]; } prev = k; } };
    chain({A0, A1, A2}); chain({B0, B1, B2, B3});
    kfs[C0].bImu = false;
    for (int j = 0; j < 4; ++j) { mps[j].mnId = j; mps[j].mWorldPos = Eigen::Vector3f(1.f + j, 2.f + j, 5.f + j); }
    mps[3].mbBad = true;
    auto see = [&](int k, int j, int idx, float ur = -1.f) { kfs[k].mvpMapPoints[idx] = &mps[j]; kfs[k].mvuRight[idx] = ur; mps[j].mObservations[&kfs[k]] = std::make_tuple(idx, -1); };
    see(A2, 0, 0); see(B2, 0, 1); see(C0, 0, 2);          // point 0: both windows and a covisible keyframe without IMU
    see(A2, 2, 1); see(D, 2, 0);                          // point 2: the covisible keyframe newer than the current one (selected, its edge skipped)
    see(A1, 1, 0); see(B1, 1, 3, 77.5f); see(B0, 1, 2);   // point 1: stereo in B1, and seen by the fixed keyframe
    see(A2, 3, 2);                                        // a bad point
  }
};

// the flattened graph the stub expects: vertices (keyframes in order, with kinds), point rows, links as (row of mPrevKF, row of the keyframe, the
// keyframe whose preintegration it carries), edges as (vertex row, point row, keyframe, keypoint)
struct Link { int r1, r2, kf; };
struct Edge { int row, pt, kf, kp; };
static void expect(Scene& s, const std::vector<int>& order, const std::vector<uint8_t>& kinds, const std::vector<int>& points, const std::vector<Link>& links,
                   const std::vector<Edge>& edges) {
  Expect& x = g_expect;
  x = Expect();
  for (int k : order) {
    const MIKeyFrame& K = s.kfs[k];
    for (int i = 0; i < 9; ++i) x.kfState.push_back(K.mRwb.m[i]);
    for (int c = 0; c < 3; ++c) x.kfState.push_back(K.mOwb.v[c]);
    for (int c = 0; c < 3; ++c) x.kfState.push_back(K.mVw.v[c]);
    const IMU::Bias& b = K.mImuBias;
    for (float v : {b.bwx, b.bwy, b.bwz, b.bax, b.bay, b.baz}) x.kfState.push_back(v);
  }
  x.kfKind = kinds;
  for (int j : points) for (int c = 0; c < 3; ++c) x.mpPos.push_back(s.mps[j].mWorldPos(c));
  for (const Link& l : links) { x.iKF1.push_back(l.r1); x.iKF2.push_back(l.r2); x.preDT.push_back(s.pre[l.kf].dT); }
  for (const Edge& e : edges) {
    x.eKF.push_back(e.row); x.eMP.push_back(e.pt);
    const cv::KeyPoint& kp = s.kfs[e.kf].mvKeysUn[e.kp];
    x.eObs.push_back(kp.pt.x); x.eObs.push_back(kp.pt.y); x.eObs.push_back(s.kfs[e.kf].mvuRight[e.kp] < 0 ? -1.f : s.kfs[e.kf].mvuRight[e.kp]);
    x.eInv.push_back(s.kfs[e.kf].mvInvLevelSigma2[kp.octave]);
  }
  const float cam[5] = {458.f, 457.f, 367.f, 248.f, 50.f};
  std::memcpy(x.cam, cam, sizeof cam);
}

int main() {
  // windows: current A2, A1 with the head A0 (covisible list, 15 unknowns: a link hangs on it); merge B2, B1, then B0 falls out as the fixed
  // keyframe, then B3.  Vertices: A2 A1 B2 B1 B3 | A0 D C0 | B0.  Points in the order the windows' matches give them: 0, 2, 1.
  const int order[9] = {A2, A1, B2, B1, B3, A0, D, C0, B0};
  {
    Scene s;
    // links in the order of the window: A1->A2, A0->A1, B1->B2, B0->B1, B2->B3, each with the later keyframe's preintegration; edges by point,
    // observations by keyframe address: point 0 <- A2, B2, C0; point 2 <- A2 (D is newer: skipped); point 1 <- A1, B0, B1 (stereo)
    expect(s, std::vector<int>(order, order + 9), {0, 0, 0, 0, 0, 0, 3, 3, 1}, {0, 2, 1}, {{1, 0, A2}, {5, 1, A1}, {3, 2, B2}, {8, 3, B1}, {2, 4, B3}},
           {{0, 0, A2, 0}, {2, 0, B2, 1}, {7, 0, C0, 2}, {0, 1, A2, 1}, {1, 2, A1, 0}, {8, 2, B0, 2}, {3, 2, B1, 3}});
    g_erase = {0, 1, 0, 0, 0, 1, 0};   // erase (B2, point 0) and (B0, point 1)
    g_calls = g_bad = 0;
    MIKeyFrame *mpCurrentKF = &s.kfs[A2], *mpMergeMatchedKF = &s.kfs[B2];
    MIMap* pCurrentMap = &s.map;
    std::map<MIKeyFrame*, g2o::Sim3> vCorrectedSim3;
    bool bStop = false;
    // src/LoopClosing.cc:1649-1650, unedited
    Optimizer::MergeInertialBA(mpCurrentKF, mpMergeMatchedKF, &bStop,
                               pCurrentMap, vCorrectedSim3);
    REQUIRE(g_calls == 1 && g_bad == 0);
    const long unsigned int id = s.kfs[A2].mnId;
    for (int k = 0; k < NKF; ++k) {
      REQUIRE(s.kfs[k].mnBALocalForKF == (k == B0 ? 0 : id));
      REQUIRE(s.kfs[k].mnBAFixedForKF == (k == B0 ? id : 0));
    }
    for (int j = 0; j < 4; ++j) REQUIRE(s.mps[j].mnBALocalForKF == (j == 3 ? 0 : id));
    // SetNewBias(mPrevKF->GetImuBias()) on the preintegration of every keyframe of the windows that has a link
    for (int k : {A2, A1, B2, B1, B3}) REQUIRE(s.pre[k].nSetNewBias == 1 && s.pre[k].last.bax == 0.1f + (k - 1));   // (the predecessor's bias as it was before the write-back)
    for (int k : {A0, B0, C0, D}) REQUIRE(s.pre[k].nSetNewBias == 0);
    // poses of every free keyframe (Tbc = I, Rwb = I: tcw = -twb), velocity and bias of the 15-unknown ones, corrPoses of all of them
    REQUIRE(vCorrectedSim3.size() == 8 && vCorrectedSim3.count(&s.kfs[B0]) == 0);
    for (int row = 0; row < 9; ++row) {
      MIKeyFrame& K = s.kfs[order[row]];
      const bool free15 = row < 6, free = row < 8;
      REQUIRE(K.nSetPose == (free ? 1 : 0) && K.nSetVelocity == (free15 ? 1 : 0) && K.nSetNewBias == (free15 ? 1 : 0));
      if (!free) continue;
      for (int c = 0; c < 3; ++c) REQUIRE(K.mTcw.t[c] == -(100.f + 21 * row + 9 + c));
      const g2o::Sim3& S = vCorrectedSim3[&K];
      REQUIRE(S.scale() == 1.0 && S.rotation().w() == 1.0 && S.rotation().x() == 0.0);
      for (int c = 0; c < 3; ++c) REQUIRE(S.translation()(c) == (double)K.mTcw.t[c]);
      if (free15) {
        REQUIRE(K.mVw(0) == 100.f + 21 * row + 12 && K.mVw(2) == 100.f + 21 * row + 14);
        REQUIRE(K.mImuBias.bwx == 100.f + 21 * row + 15 && K.mImuBias.bwz == 100.f + 21 * row + 17 && K.mImuBias.bax == 100.f + 21 * row + 18 && K.mImuBias.baz == 100.f + 21 * row + 20);
      }
    }
    REQUIRE(s.kfs[D].mVw(0) == 0.1f * D && s.kfs[C0].mImuBias.bax == 0.1f + C0 && s.kfs[B0].mOwb(0) == 0.5f * B0);
    // points 0, 2, 1 <- rows 0, 1, 2
    const int rows[3] = {0, 2, 1};
    for (int r = 0; r < 3; ++r) {
      const MIMapPoint& p = s.mps[rows[r]];
      REQUIRE(p.nSetPos == 1 && p.nUpdates == 1 && p.mWorldPos.v[0] == 200.f + 3 * r && p.mWorldPos.v[2] == 202.f + 3 * r);
    }
    REQUIRE(s.mps[3].nSetPos == 0 && s.mps[3].nUpdates == 0);
    // erased: both sides of the two observations, nothing else
    REQUIRE(s.kfs[B2].mvpMapPoints[1] == nullptr && s.mps[0].mObservations.count(&s.kfs[B2]) == 0);
    REQUIRE(s.kfs[B0].mvpMapPoints[2] == nullptr && s.mps[1].mObservations.count(&s.kfs[B0]) == 0);
    REQUIRE(s.kfs[A2].mvpMapPoints[0] == &s.mps[0] && s.kfs[C0].mvpMapPoints[2] == &s.mps[0] && s.kfs[B1].mvpMapPoints[3] == &s.mps[1]);
    REQUIRE(s.mps[0].mObservations.size() == 2 && s.mps[1].mObservations.size() == 2 && s.mps[2].mObservations.size() == 2);
    REQUIRE(s.map.changes == 1);
  }
  {   // *pbStopFlag set: the graph is selected and marked, the preintegrations take their bias, nothing reaches the device, nothing is written (:4276)
    Scene s;
    g_calls = g_bad = 0;
    std::map<MIKeyFrame*, g2o::Sim3> corr;
    bool bStop = true;
    Optimizer::MergeInertialBA(&s.kfs[A2], &s.kfs[B2], &bStop, &s.map, corr);
    REQUIRE(g_calls == 0 && corr.empty() && s.map.changes == 0);
    REQUIRE(s.kfs[A0].mnBALocalForKF == s.kfs[A2].mnId && s.kfs[B0].mnBAFixedForKF == s.kfs[A2].mnId && s.pre[A2].nSetNewBias == 1);
    for (int k = 0; k < NKF; ++k) REQUIRE(s.kfs[k].nSetPose == 0 && s.kfs[k].nSetVelocity == 0);
    for (int j = 0; j < 4; ++j) REQUIRE(s.mps[j].nSetPos == 0 && s.mps[j].nUpdates == 0);
  }
  {   // a current chain of one keyframe: it moves to the covisible list and no link hangs on it — free in the pose only.  Windows: B2, B1, B3 with
    // B0 fixed; points 0 (B2) and 1 (B1); covisible: A2, then C0 for point 0 and A1 for point 1.  Vertices: B2 B1 B3 | A2 C0 A1 | B0.
    Scene s;
    s.kfs[A2].mPrevKF = nullptr;
    expect(s, {B2, B1, B3, A2, C0, A1, B0}, {0, 0, 0, 3, 3, 3, 1}, {0, 1}, {{1, 0, B2}, {6, 1, B1}, {0, 2, B3}},
           {{3, 0, A2, 0}, {0, 0, B2, 1}, {4, 0, C0, 2}, {5, 1, A1, 0}, {6, 1, B0, 2}, {1, 1, B1, 3}});
    g_erase.clear();
    g_calls = g_bad = 0;
    std::map<MIKeyFrame*, g2o::Sim3> corr;
    bool bStop = false;
    Optimizer::MergeInertialBA(&s.kfs[A2], &s.kfs[B2], &bStop, &s.map, corr);
    REQUIRE(g_calls == 1 && g_bad == 0);
    REQUIRE(s.kfs[A0].mnBALocalForKF == 0 && s.kfs[A1].mnBALocalForKF == s.kfs[A2].mnId && s.kfs[D].mnBALocalForKF == 0);
    for (int k : {A2, C0, A1}) REQUIRE(s.kfs[k].nSetPose == 1 && s.kfs[k].nSetVelocity == 0 && s.kfs[k].nSetNewBias == 0 && corr.count(&s.kfs[k]) == 1);
    for (int k : {B2, B1, B3}) REQUIRE(s.kfs[k].nSetPose == 1 && s.kfs[k].nSetVelocity == 1 && corr.count(&s.kfs[k]) == 1);
    REQUIRE(s.pre[A2].nSetNewBias == 0 && s.pre[A1].nSetNewBias == 0 && corr.size() == 6 && s.mps[2].nSetPos == 0);
  }
  {   // windows that see no point: nothing for the device; corrPoses of every keyframe of the windows from its pose as it stands, the change index
    Scene s;
    for (auto& K : s.kfs) for (auto& m : K.mvpMapPoints) m = nullptr;
    g_calls = g_bad = 0;
    std::map<MIKeyFrame*, g2o::Sim3> corr;
    bool bStop = false;
    s.kfs[A1].mTcw.t[0] = 7.f;
    Optimizer::MergeInertialBA(&s.kfs[A2], &s.kfs[B2], &bStop, &s.map, corr);
    REQUIRE(g_calls == 0 && s.map.changes == 1 && corr.size() == 6);   // A2 A1 B2 B1 B3 and the head A0
    REQUIRE(corr.count(&s.kfs[B0]) == 0 && corr[&s.kfs[A1]].translation()(0) == 7.0 && corr[&s.kfs[A1]].scale() == 1.0);
    for (int k = 0; k < NKF; ++k) REQUIRE(s.kfs[k].nSetPose == 0 && s.kfs[k].nSetVelocity == 0);
  }
  std::printf("merge inertial ba member ok\n");
  return 0;
}
