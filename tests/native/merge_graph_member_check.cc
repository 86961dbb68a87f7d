// The reference-typed Optimizer::OptimizeEssentialGraph(pCurKF, vpFixedKFs, vpFixedCorrectedKFs, vpNonFixedKFs, vpNonCorrectedMPs) of
// include/morb/Optimizer_reference.h on a mock map (tests/native/mock_merge_graph).  Ten keyframes k0 .. k9 with mnId 1, 3, .. 19: k0 and k1 are
// the merged map's (vpFixedKFs, handed over unsorted), k2 .. k7 the old map's (vpNonFixedKFs), k6 and k7 its window (vpFixedCorrectedKFs, so both
// are in two lists), k4 is bad and k5's parent, k8 is in no list, k9 lies beyond GetMaxKFid().  The window's spanning tree hangs from the merged
// map (k7's parent is k1, k6's parent is k7, so k6 is k7's child and a covisible of it).  Covisibles below weight 100, of a larger mnId, that are
// the parent, a child or a loop edge are left out; an old loop edge is seen from its later end only; k2 is covisible with k0 of the other map,
// a candidate that the entry's good / bad rule drops.  Points: references in vpNonFixedKFs, behind a bad observer, in the window, in
// vpFixedKFs (the point stays), in no list, beyond GetMaxKFid(), none at all, and a bad point.
//   -DMG_STUB_ENTRY (tests/test_merge_graph_cpu.py, -fsanitize=address,undefined, no library, no GPU): the C entry is a stub that checks the
//   flattened problem against the expectation written out below and returns canned results; the write-back is checked.
//   Otherwise (tests/test_merge_graph_adapter_gpu.py): `merge_graph_member_check <problem.bin> <result.bin>` dumps the flattened problem in
//   merge_graph_adapter_check.cc's layout, runs the member on the library, and dumps every keyframe's pose and BefMerge members and every
//   point's position.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "merge_graph_mock.h"
#include "Optimizer.h"

using namespace ORB_SLAM3;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
template <class T> static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), n * sizeof(T)); }

static MGSE3 pose_of(double angle, float x, float y, float z) {   // a rotation of `angle` rad about (0.2, 0.9, -0.1), as a float unit quaternion
  const double h = std::sin(angle / 2), n = std::sqrt(0.04 + 0.81 + 0.01);
  float q[4] = {(float)(0.2 / n * h), (float)(0.9 / n * h), (float)(-0.1 / n * h), (float)std::cos(angle / 2)};
  const float len = std::sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]));
  for (float& c : q) c /= len;
  return MGSE3(MGQuat(q[3], q[0], q[1], q[2]), MGVec3(x, y, z));
}

struct Scene {
  MGMap map;
  std::vector<MGKeyFrame> kfs;
  std::vector<MGMapPoint> mps;
  std::vector<MGKeyFrame*> vpFixedKFs, vpFixedCorrectedKFs, vpNonFixedKFs;
  std::vector<MGMapPoint*> vpNonCorrectedMPs;
  Scene() : kfs(10), mps(8) {
    map.maxKFid = 17;
    for (int k = 0; k < 10; ++k) {
      MGKeyFrame& K = kfs[k];
      K.mnId = 2 * k + 1; K.mpMap = &map;
      K.mTcw = pose_of(0.12 * k, 0.8f * k, 0.05f * k * k, -0.3f * k);
      K.mTwc = K.mTcw.inverse();
    }
    for (int k : {6, 7}) {   // the window: the pose before the merge, and its inverse, as MergeLocal stored them
      kfs[k].mTcwBefMerge = pose_of(0.12 * k + 0.05, 0.8f * k + 0.4f, 0.05f * k * k - 0.1f, -0.3f * k + 0.25f);
      kfs[k].mTwcBefMerge = kfs[k].mTcwBefMerge.inverse();
    }
    kfs[4].mbBad = true;
    auto tree = [&](int c, int p) { kfs[c].parent = &kfs[p]; kfs[p].children.insert(&kfs[c]); };
    tree(1, 0); tree(3, 2); tree(4, 3); tree(5, 4); tree(6, 7); tree(7, 1);
    auto cov = [&](int a, std::vector<std::pair<int, int>> l) { for (auto& kw : l) kfs[a].covisibles.push_back({&kfs[kw.first], kw.second}); };
    cov(1, {{0, 300}});                                    // its parent
    cov(2, {{0, 120}});                                    // a keyframe of the other map: a candidate, dropped by the rule
    cov(3, {{2, 200}});                                    // its parent
    cov(5, {{4, 250}, {3, 150}, {6, 120}, {2, 90}});       // the bad parent; an edge; larger mnId; below 100
    cov(6, {{7, 300}, {5, 200}, {1, 130}, {3, 110}});      // parent; an edge; an edge into the merged map; a loop edge
    cov(7, {{6, 280}, {1, 260}, {0, 150}, {5, 140}});      // its child; parent; an edge into the merged map; an edge
    auto loop = [&](int a, int b) { kfs[a].loopEdges.insert(&kfs[b]); kfs[b].loopEdges.insert(&kfs[a]); };
    loop(5, 2); loop(6, 3);
    vpFixedKFs = {&kfs[1], &kfs[0]};
    vpFixedCorrectedKFs = {&kfs[7], &kfs[6]};
    for (int k = 2; k <= 7; ++k) vpNonFixedKFs.push_back(&kfs[k]);
    for (int j = 0; j < 8; ++j) { mps[j].mnId = j; mps[j].mWorldPos = MGVec3(1.f + j, 0.5f * j, 4.f - 0.3f * j); vpNonCorrectedMPs.push_back(&mps[j]); }
    mps[0].observers = {&kfs[3]};
    mps[1].observers = {&kfs[4], &kfs[5]};   // behind the bad keyframe
    mps[2].observers = {&kfs[2]}; mps[2].mbBad = true;
    mps[3].observers = {&kfs[0]};            // vpFixedKFs: stays
    mps[4].observers = {&kfs[6]};
    mps[5].observers = {};                   // no reference keyframe
    mps[6].observers = {&kfs[8]};            // in no list
    mps[7].observers = {&kfs[9]};            // beyond GetMaxKFid()
  }
};

static const int kRowKF[7] = {0, 1, 2, 3, 5, 6, 7};   // vertex -> keyframe (k4 is bad)

#ifdef MG_STUB_ENTRY
static int g_calls = 0, g_bad = 0;
static Scene* g_scene = nullptr;
extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
int morb_optimizer_create(morb_optimizer** out, int) { static int token; *out = reinterpret_cast<morb_optimizer*>(&token); return MORB_OK; }
int morb_optimizer_set_exact_order(morb_optimizer*, int) { return MORB_OK; }
const char* morb_last_error(void) { return "stub"; }
int morb_optimize_essential_graph_merge(morb_optimizer*, int nKF, const uint8_t* kfLists, float* kfTcw, float* kfTwc, float* kfTcwBefMerge, float* kfTwcBefMerge,
                                        int nC, const int* cI, const int* cJ, uint8_t* cKept, int nMP, float* mpPos, const int* mpRef, int* stats4, double* chi2) {
  ++g_calls;
  // the expectation, written out by hand.  Vertices in ascending mnId: k0 k1 k2 k3 k5 k6 k7 -> 0 .. 6
  const uint8_t lists[7] = {1, 1, 4, 4, 4, 6, 6};
  const int edges[19][2] = {{1, 0},                                  // k1: parent (k0 has no candidate)
                            {6, 1}, {6, 0}, {6, 4},                  // k7 as a window keyframe: parent k1, covisibles k0 and k5 (k6 is its child)
                            {5, 6}, {5, 3}, {5, 4}, {5, 1},          // k6 as a window keyframe: parent k7, loop edge k3, covisibles k5 and k1
                            {2, 0},                                  // k2: covisible k0
                            {3, 2},                                  // k3: parent
                            {4, 2}, {4, 3},                          // k5: (parent k4 is bad) loop edge k2, covisible k3
                            {5, 6}, {5, 3}, {5, 4}, {5, 1},          // k6 again, as a non-fixed keyframe
                            {6, 1}, {6, 0}, {6, 4}};                 // k7 again
  const int refs[8] = {3, 4, -1, 0, 5, -1, -1, -1};
  if (nKF != 7 || std::memcmp(kfLists, lists, 7) != 0) { ++g_bad; std::printf("vertices differ\n"); return MORB_ERR_INVALID; }
  if (nC != 19) { ++g_bad; std::printf("%d candidates\n", nC); }
  for (int c = 0; c < nC && c < 19; ++c)
    if (cI[c] != edges[c][0] || cJ[c] != edges[c][1]) { ++g_bad; std::printf("candidate %d is (%d, %d)\n", c, cI[c], cJ[c]); }
  if (nMP != 8 || std::memcmp(mpRef, refs, sizeof refs) != 0) { ++g_bad; std::printf("point references differ\n"); }
  for (int v = 0; v < 7; ++v) {
    const MGKeyFrame& K = g_scene->kfs[kRowKF[v]];
    const MGSE3* T[4] = {&K.mTcw, &K.mTwc, &K.mTcwBefMerge, &K.mTwcBefMerge};
    const float* got[4] = {kfTcw + 7 * v, kfTwc + 7 * v, kfTcwBefMerge + 7 * v, kfTwcBefMerge + 7 * v};
    for (int a = 0; a < 4; ++a)
      if (std::memcmp(got[a], T[a]->q.q, 16) != 0 || std::memcmp(got[a] + 4, T[a]->t.v, 12) != 0) { ++g_bad; std::printf("pose %d of vertex %d differs\n", a, v); }
  }
  for (int m = 0; m < 8; ++m)
    if (refs[m] >= 0 && std::memcmp(mpPos + 3 * m, g_scene->mps[m].mWorldPos.v, 12) != 0) { ++g_bad; std::printf("point %d differs\n", m); }
  // canned results
  for (int c = 0; c < nC; ++c) cKept[c] = c != 8;
  for (int v = 0; v < 7; ++v) {
    if (!(kfLists[v] & 4)) continue;
    std::memcpy(kfTcwBefMerge + 7 * v, kfTcw + 7 * v, 28); std::memcpy(kfTwcBefMerge + 7 * v, kfTwc + 7 * v, 28);
    const float p[7] = {0.f, 0.6f, 0.f, 0.8f, 10.f + v, 20.f + v, 30.f + v};
    std::memcpy(kfTcw + 7 * v, p, sizeof p);
  }
  for (int i = 0; i < nMP * 3; ++i) mpPos[i] = 200.f + i;
  const int s[4] = {3, 3, 3, 5};
  std::memcpy(stats4, s, sizeof s);
  chi2[0] = 2; chi2[1] = 1;
  return MORB_OK;
}
}
#endif

int main(int argc, char** argv) {
  Scene sc;
  MGKeyFrame* mpCurrentKF = &sc.kfs[7];
  auto &vpMergeConnectedKFs = sc.vpFixedKFs, &vpLocalCurrentWindowKFs = sc.vpFixedCorrectedKFs, &vpCurrentMapKFs = sc.vpNonFixedKFs;
  auto& vpCurrentMapMPs = sc.vpNonCorrectedMPs;
  const Scene before;
#ifdef MG_STUB_ENTRY
  (void)argc; (void)argv;
  g_scene = &sc;
      Optimizer::OptimizeEssentialGraph(mpCurrentKF, vpMergeConnectedKFs,
                                        vpLocalCurrentWindowKFs,
                                        vpCurrentMapKFs, vpCurrentMapMPs);
  REQUIRE(g_calls == 1 && g_bad == 0);
  auto same = [](const MGSE3& a, const MGSE3& b) { return std::memcmp(a.q.q, b.q.q, 16) == 0 && std::memcmp(a.t.v, b.t.v, 12) == 0; };
  const int rowOf[10] = {0, 1, 2, 3, -1, 4, 5, 6, -1, -1};
  for (int k = 0; k < 10; ++k) {
    const bool tail = k >= 2 && k <= 7 && k != 4;   // the keyframes of vpNonFixedKFs that are not bad, the window's two included
    REQUIRE(sc.kfs[k].nSetPose == (tail ? 1 : 0));
    if (!tail) { REQUIRE(same(sc.kfs[k].mTcw, before.kfs[k].mTcw) && same(sc.kfs[k].mTcwBefMerge, before.kfs[k].mTcwBefMerge)); continue; }
    REQUIRE(same(sc.kfs[k].mTcwBefMerge, before.kfs[k].mTcw) && same(sc.kfs[k].mTwcBefMerge, before.kfs[k].mTwc));
    REQUIRE(sc.kfs[k].mTcw.q.q[1] == 0.6f && sc.kfs[k].mTcw.q.q[3] == 0.8f && sc.kfs[k].mTcw.t.v[0] == 10.f + rowOf[k] && sc.kfs[k].mTcw.t.v[2] == 30.f + rowOf[k]);
  }
  for (int j = 0; j < 8; ++j) {
    const bool moved = j == 0 || j == 1 || j == 4;
    REQUIRE(sc.mps[j].nSetPos == (moved ? 1 : 0) && sc.mps[j].nUpdates == (moved ? 1 : 0));
    if (moved) REQUIRE(sc.mps[j].mWorldPos.v[1] == 200.f + 3 * j + 1);
    else REQUIRE(sc.mps[j].mWorldPos.v[1] == before.mps[j].mWorldPos.v[1]);
  }
  REQUIRE(sc.mps[1].nErased == 1 && sc.mps[1].GetReferenceKeyFrame() == &sc.kfs[5]);
  std::printf("merge graph member ok\n");
  return 0;
#else
  if (argc < 3) { std::printf("usage: %s problem.bin result.bin\n", argv[0]); return 2; }
  {
    Scene copy;
    MergeGraphFlat f;
    morb_glue::flatten_merge_graph(&copy.kfs[7], copy.vpFixedKFs, copy.vpFixedCorrectedKFs, copy.vpNonFixedKFs, copy.vpNonCorrectedMPs, f);
    std::ofstream out(argv[1], std::ios::binary);
    const int hd[3] = {(int)f.kfLists.size(), (int)f.cI.size(), (int)f.mpRef.size()};
    wr(out, hd, 3); wr(out, f.kfLists.data(), f.kfLists.size());
    wr(out, f.kfTcw.data(), f.kfTcw.size()); wr(out, f.kfTwc.data(), f.kfTwc.size()); wr(out, f.kfTcwBefMerge.data(), f.kfTcwBefMerge.size());
    wr(out, f.kfTwcBefMerge.data(), f.kfTwcBefMerge.size());
    wr(out, f.cI.data(), f.cI.size()); wr(out, f.cJ.data(), f.cJ.size()); wr(out, f.mpPos.data(), f.mpPos.size()); wr(out, f.mpRef.data(), f.mpRef.size());
  }
      Optimizer::OptimizeEssentialGraph(mpCurrentKF, vpMergeConnectedKFs,
                                        vpLocalCurrentWindowKFs,
                                        vpCurrentMapKFs, vpCurrentMapMPs);
  std::ofstream out(argv[2], std::ios::binary);
  for (int k = 0; k < 10; ++k)
    for (const MGSE3* T : {&sc.kfs[k].mTcw, &sc.kfs[k].mTcwBefMerge, &sc.kfs[k].mTwcBefMerge}) { wr(out, T->q.q, 4); wr(out, T->t.v, 3); }
  for (int j = 0; j < 8; ++j) wr(out, sc.mps[j].mWorldPos.v, 3);
  for (int k = 0; k < 10; ++k) wr(out, &sc.kfs[k].nSetPose, 1);
  return out ? 0 : 1;
#endif
}
