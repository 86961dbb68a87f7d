// The reference-typed Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale) of
// include/morb/Optimizer_reference.h on a mock map (tests/native/mock_essential_graph), with the call expression of LoopClosing::CorrectLoop
// (src/LoopClosing.cc:1206-1208) unedited.  Seven keyframes k0 .. k6 with mnId 1, 3, .. 13; k0 is the map's initial keyframe, k3 is bad, k6 the
// current and k1 the loop keyframe; k5 and k6 carry corrected and non-corrected Sim3.  The map exercises every condition of
// Optimizer.cc:1514-1682: a LoopConnections weight below 100 on the (cur, loop) pair (kept) and off it (dropped), a connection to the bad
// keyframe (no edge, but its pair enters sInsertedEdges), covisibles that are the parent, a child, bad, of a larger mnId or already in
// sInsertedEdges, an old loop edge seen from both ends, an IMU link that doubles the spanning-tree edge and one to the bad keyframe.
//   -DEG_STUB_ENTRY (tests/test_essential_graph_cpu.py, -fsanitize=address,undefined, no library, no GPU): the C entry is a stub that
//   checks the flattened graph against the expectation written out below and returns canned results; the write-back is checked.
//   Otherwise (tests/test_essential_graph_adapter_gpu.py): `essential_graph_member_check <problem.bin> <result.bin>` dumps the flattened
//   problem in essential_graph_adapter_check.cc's layout, runs the member on the library, and dumps every keyframe's pose (7 floats) and
//   every point's position.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "essential_graph_mock.h"
#include "Optimizer.h"

using namespace ORB_SLAM3;
std::mutex ORB_SLAM3::MapPoint::mGlobalMutex;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
template <class T> static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), n * sizeof(T)); }

struct Scene {
  EGMap map;
  std::vector<EGKeyFrame> kfs;
  std::vector<EGMapPoint> mps;
  std::map<EGKeyFrame*, EGSim3> NonCorrectedSim3, CorrectedSim3;
  std::map<EGKeyFrame*, std::set<EGKeyFrame*>> LoopConnections;
  static EGSim3 pose_sim3(const EGKeyFrame& K) {
    EGVec3 t;
    for (int c = 0; c < 3; ++c) t.v[c] = (double)K.mTcw.t[c];
    return EGSim3(EGQuat((double)K.mTcw.q[3], (double)K.mTcw.q[0], (double)K.mTcw.q[1], (double)K.mTcw.q[2]), t, 1.0);
  }
  Scene() : kfs(7), mps(5) {
    map.initKF = 1;
    for (int k = 0; k < 7; ++k) {
      EGKeyFrame& K = kfs[k];
      K.mnId = 2 * k + 1; K.mpMap = &map;
      const double a = 0.12 * k, h = std::sin(a / 2), n = std::sqrt(0.04 + 0.81 + 0.01);   // a rotation of 0.12 k rad about (0.2, 0.9, -0.1)
      K.mTcw.q[0] = (float)(0.2 / n * h); K.mTcw.q[1] = (float)(0.9 / n * h); K.mTcw.q[2] = (float)(-0.1 / n * h); K.mTcw.q[3] = (float)std::cos(a / 2);
      K.mTcw.t[0] = 0.8f * k; K.mTcw.t[1] = 0.05f * k * k; K.mTcw.t[2] = -0.3f * k;
    }
    kfs[3].mbBad = true;
    const int order[7] = {0, 2, 1, 3, 4, 5, 6};   // GetAllKeyFrames() is not sorted by mnId
    for (int k : order) map.kfs.push_back(&kfs[k]);
    auto tree = [&](int c, int p) { kfs[c].parent = &kfs[p]; kfs[p].children.insert(&kfs[c]); };
    tree(1, 0); tree(2, 1); tree(3, 2); tree(4, 2); tree(5, 4); tree(6, 5);
    auto cov = [&](int a, std::vector<std::pair<int, int>> l) { for (auto& kw : l) { kfs[a].covisibles.push_back(&kfs[kw.first]); kfs[a].weights[&kfs[kw.first]] = kw.second; } };
    cov(0, {{1, 300}});                                  // its child
    cov(1, {{0, 300}});                                  // its parent
    cov(2, {{1, 250}, {0, 150}, {4, 90}});               // parent; an edge; below 100
    cov(4, {{2, 260}, {3, 240}, {5, 200}, {1, 120}});    // parent; bad; larger mnId; an edge
    cov(5, {{4, 270}, {6, 220}, {2, 110}});              // parent; its child; an edge
    cov(6, {{5, 280}, {2, 140}, {4, 130}, {1, 105}});    // parent; in sInsertedEdges; an edge; in sInsertedEdges
    kfs[4].loopEdges.insert(&kfs[0]); kfs[0].loopEdges.insert(&kfs[4]);   // an old loop: an edge from k4 only
    kfs[2].bImu = true; kfs[2].mPrevKF = &kfs[1];        // doubles the spanning-tree edge
    kfs[5].bImu = true; kfs[5].mPrevKF = &kfs[3];        // to the bad keyframe: dropped
    kfs[6].weights[&kfs[1]] = 30; kfs[6].weights[&kfs[0]] = 40; kfs[5].weights[&kfs[1]] = 50; kfs[5].weights[&kfs[0]] = 100; kfs[5].weights[&kfs[3]] = 150;
    LoopConnections[&kfs[6]] = {&kfs[1], &kfs[0], &kfs[2]};   // (cur, loop) at weight 30: kept; k0 at 40: dropped; k2 at 140: kept
    LoopConnections[&kfs[5]] = {&kfs[1], &kfs[0], &kfs[3]};   // k1 at 50: dropped; k0 at 100: kept; k3 is bad: no edge
    // CorrectLoop's propagation (LoopClosing.cc:1060-1090): the current keyframe's corrected Sim3, and Sic * it for its neighbour
    EGVec3 gt; gt.v[0] = 0.15; gt.v[1] = -0.05; gt.v[2] = 0.2;
    const EGSim3 G(EGQuat(std::cos(0.02), 0.3 * std::sin(0.02), 0.9 * std::sin(0.02), -0.316227766 * std::sin(0.02)), gt, 1.03);
    const EGSim3 S6 = pose_sim3(kfs[6]), S5 = pose_sim3(kfs[5]);
    NonCorrectedSim3[&kfs[6]] = S6; NonCorrectedSim3[&kfs[5]] = S5;
    CorrectedSim3[&kfs[6]] = G * S6; CorrectedSim3[&kfs[5]] = (S5 * S6.inverse()) * (G * S6);
    for (int j = 0; j < 5; ++j) { mps[j].mnId = j; mps[j].mpMap = &map; mps[j].mWorldPos = Eigen::Vector3f(1.f + j, 0.5f * j, 4.f - 0.3f * j); map.mps.push_back(&mps[j]); }
    mps[0].ref = &kfs[2];
    mps[1].ref = &kfs[4]; mps[1].mnCorrectedByKF = kfs[6].mnId; mps[1].mnCorrectedReference = kfs[5].mnId;   // corrected through k5, not its reference keyframe
    mps[2].ref = &kfs[1]; mps[2].mbBad = true;
    mps[3].ref = &kfs[6];
    mps[4].ref = &kfs[0];
  }
};

#ifdef EG_STUB_ENTRY
static int g_calls = 0, g_bad = 0;
struct Expect { std::vector<double> kfSim3, eSji; std::vector<uint8_t> kfFlags; std::vector<int> eI, eJ, mpRef; std::vector<float> mpPos; } g_expect;
extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
int morb_optimizer_create(morb_optimizer** out, int) { static int token; *out = reinterpret_cast<morb_optimizer*>(&token); return MORB_OK; }
int morb_optimizer_set_exact_order(morb_optimizer*, int) { return MORB_OK; }
const char* morb_last_error(void) { return "stub"; }
int morb_optimize_essential_graph(morb_optimizer*, int nKF, double* kfSim3, const uint8_t* kfFlags, int nE, const int* eI, const int* eJ, const double* eSji, int nMP,
                                  float* mpPos, const int* mpRef, int* stats4, double* chi2) {
  ++g_calls;
  const Expect& x = g_expect;
  auto same = [](const auto& v, const auto* p, size_t n) { return v.size() == n && (n == 0 || std::memcmp(v.data(), p, n * sizeof(v[0])) == 0); };
  if (!same(x.kfFlags, kfFlags, nKF)) { ++g_bad; std::printf("flags differ\n"); }
  if (!same(x.kfSim3, kfSim3, (size_t)nKF * 8)) { ++g_bad; std::printf("estimates differ\n"); }
  if (!same(x.eI, eI, nE) || !same(x.eJ, eJ, nE)) {
    ++g_bad; std::printf("edge list differs:");
    for (int e = 0; e < nE; ++e) std::printf(" (%d,%d)", eI[e], eJ[e]);
    std::printf("\n");
  } else if (!same(x.eSji, eSji, (size_t)nE * 8)) { ++g_bad; std::printf("measurements differ\n"); }
  if (!same(x.mpRef, mpRef, nMP) || !same(x.mpPos, mpPos, (size_t)nMP * 3)) { ++g_bad; std::printf("points differ\n"); }
  for (int v = 0; v < nKF; ++v) {   // canned: quaternion 0.1 v .., translation 10 + v .., scale 2
    double* S = kfSim3 + 8 * v;
    S[0] = 0.01 * v; S[1] = 0.02; S[2] = 0.03; S[3] = 0.99; S[4] = 10.0 + v; S[5] = 20.0 + v; S[6] = 30.0 + v; S[7] = 2.0;
  }
  for (int i = 0; i < nMP * 3; ++i) mpPos[i] = 200.f + i;
  const int s[4] = {2, 11, nKF - 1, 9};
  std::memcpy(stats4, s, sizeof s);
  chi2[0] = 1; chi2[1] = 0.5;
  return MORB_OK;
}
}
#endif

int main(int argc, char** argv) {
  Scene sc;
  EGMap* pLoopMap = &sc.map;
  EGKeyFrame *mpLoopMatchedKF = &sc.kfs[1], *mpCurrentKF = &sc.kfs[6];
  auto& NonCorrectedSim3 = sc.NonCorrectedSim3; auto& CorrectedSim3 = sc.CorrectedSim3; auto& LoopConnections = sc.LoopConnections;
  bool bFixedScale = false;
#ifdef EG_STUB_ENTRY
  (void)argc; (void)argv;
  {   // the expectation, written out by hand.  Vertices in ascending mnId: k0 k1 k2 k4 k5 k6 -> 0 .. 5
    Expect& x = g_expect;
    EGKeyFrame* byRow[6] = {&sc.kfs[0], &sc.kfs[1], &sc.kfs[2], &sc.kfs[4], &sc.kfs[5], &sc.kfs[6]};
    std::vector<EGSim3> V(6), N(6);   // vScw, and what a normal edge takes: NonCorrectedSim3's entry or vScw
    for (int r = 0; r < 6; ++r) { V[r] = r >= 4 ? sc.CorrectedSim3[byRow[r]] : Scene::pose_sim3(*byRow[r]); N[r] = r >= 4 ? sc.NonCorrectedSim3[byRow[r]] : V[r]; }
    x.kfFlags = {1, 0, 0, 0, 0, 0};
    for (int r = 0; r < 6; ++r) { double s8[8]; morb_glue::sim3_to8(V[r], s8); x.kfSim3.insert(x.kfSim3.end(), s8, s8 + 8); }
    struct E { int i, j; bool loop; };
    const E edges[] = {{4, 0, true}, {5, 1, true}, {5, 2, true},                 // LoopConnections: k5 -> k0; k6 -> k1 (the pair), k6 -> k2
                       {2, 1, false}, {2, 0, false}, {2, 1, false},              // k2: parent, covisible k0, IMU link to k1
                       {1, 0, false},                                            // k1: parent
                       {3, 2, false}, {3, 0, false}, {3, 1, false},              // k4: parent k2, old loop edge to k0, covisible k1
                       {4, 3, false}, {4, 2, false},                             // k5: parent k4, covisible k2
                       {5, 4, false}, {5, 3, false}};                            // k6: parent k5, covisible k4
    for (const E& e : edges) {
      x.eI.push_back(e.i); x.eJ.push_back(e.j);
      const EGSim3 M = e.loop ? V[e.j] * V[e.i].inverse() : N[e.j] * N[e.i].inverse();
      double s8[8]; morb_glue::sim3_to8(M, s8); x.eSji.insert(x.eSji.end(), s8, s8 + 8);
    }
    x.mpRef = {2, 4, -1, 5, 0};
    for (int j = 0; j < 5; ++j) for (int c = 0; c < 3; ++c) x.mpPos.push_back(j == 2 ? 0.f : sc.mps[j].mWorldPos.v[c]);
  }
  Optimizer::OptimizeEssentialGraph(pLoopMap, mpLoopMatchedKF, mpCurrentKF,
                                      NonCorrectedSim3, CorrectedSim3,
                                      LoopConnections, bFixedScale);
  REQUIRE(g_calls == 1 && g_bad == 0);
  const int rowOf[7] = {0, 1, 2, -1, 3, 4, 5};
  for (int k = 0; k < 7; ++k) {   // SetPose with t / s on every keyframe that has a vertex
    REQUIRE(sc.kfs[k].nSetPose == (k == 3 ? 0 : 1));
    if (k == 3) continue;
    const int v = rowOf[k];
    REQUIRE(sc.kfs[k].mTcw.q[0] == (float)(0.01 * v) && sc.kfs[k].mTcw.q[3] == 0.99f);
    REQUIRE(sc.kfs[k].mTcw.t[0] == (float)(10.0 + v) / 2.f && sc.kfs[k].mTcw.t[2] == (float)(30.0 + v) / 2.f);
  }
  for (int j = 0; j < 5; ++j) {
    REQUIRE(sc.mps[j].nSetPos == (j == 2 ? 0 : 1) && sc.mps[j].nUpdates == (j == 2 ? 0 : 1));
    if (j != 2) REQUIRE(sc.mps[j].mWorldPos.v[1] == 200.f + 3 * j + 1);
  }
  REQUIRE(sc.map.changes == 1);
  bFixedScale = true;   // _fix_scale on every vertex
  for (auto& f : g_expect.kfFlags) f |= 2;
  Scene again;
  Optimizer::OptimizeEssentialGraph(&again.map, &again.kfs[1], &again.kfs[6], again.NonCorrectedSim3, again.CorrectedSim3, again.LoopConnections, bFixedScale);
  REQUIRE(g_calls == 2 && g_bad == 0);
  std::printf("essential graph member ok\n");
  return 0;
#else
  if (argc < 3) { std::printf("usage: %s problem.bin result.bin\n", argv[0]); return 2; }
  EssentialGraphFlat f;
  morb_glue::flatten_essential_graph(pLoopMap, mpLoopMatchedKF, mpCurrentKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixedScale, f);
  {
    std::ofstream out(argv[1], std::ios::binary);
    const int hd[3] = {(int)f.kfFlags.size(), (int)f.eI.size(), (int)f.mpRef.size()};
    wr(out, hd, 3); wr(out, f.kfSim3.data(), f.kfSim3.size()); wr(out, f.kfFlags.data(), f.kfFlags.size()); wr(out, f.eI.data(), f.eI.size()); wr(out, f.eJ.data(), f.eJ.size());
    wr(out, f.eSji.data(), f.eSji.size()); wr(out, f.mpPos.data(), f.mpPos.size()); wr(out, f.mpRef.data(), f.mpRef.size());
  }
  Optimizer::OptimizeEssentialGraph(pLoopMap, mpLoopMatchedKF, mpCurrentKF,
                                      NonCorrectedSim3, CorrectedSim3,
                                      LoopConnections, bFixedScale);
  std::ofstream out(argv[2], std::ios::binary);
  for (int k = 0; k < 7; ++k) { wr(out, sc.kfs[k].mTcw.q, 4); wr(out, sc.kfs[k].mTcw.t, 3); }
  for (int j = 0; j < 5; ++j) wr(out, sc.mps[j].mWorldPos.v, 3);
  for (int k = 0; k < 7; ++k) wr(out, &sc.kfs[k].nSetPose, 1);
  return out ? 0 : 1;
#endif
}
