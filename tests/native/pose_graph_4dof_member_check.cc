// The reference-typed Optimizer::OptimizeEssentialGraph4DoF(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections) of
// include/morb/Optimizer_reference.h on a mock map (tests/native/mock_pose_graph_4dof), with the call expression of LoopClosing::CorrectLoop
// (src/LoopClosing.cc:1201-1203) unedited.  Seven keyframes k0 .. k6 with mnId 1, 3, .. 13, chained by mPrevKF / mNextKF; k3 is bad, k6 the
// current and k1 the loop keyframe (the fixed vertex); k5 and k6 carry corrected (scale 1.03) and non-corrected Sim3.  The map exercises the
// conditions of Optimizer.cc:5236-5426 and the places where the reference is undefined: a LoopConnections weight below 100 on the (cur, loop)
// pair (kept) and off it (dropped), a connection to the bad keyframe (no edge, but its pair enters sInsertedEdges), an mPrevKF link to the bad
// keyframe (dropped), covisibles that are mPrevKF, mNextKF, a child, a loop edge, bad, of a larger mnId, below 100 or already in
// sInsertedEdges, an old loop edge seen from both ends, a point whose reference keyframe is bad.
//   -DPG4_STUB_ENTRY (tests/test_pose_graph_4dof_cpu.py, -fsanitize=address,undefined, no library, no GPU): the C entry is a stub that
//   checks the flattened graph against the expectation written out below and returns canned results; the write-back is checked.
//   Otherwise (tests/test_pose_graph_4dof_adapter_gpu.py): `pose_graph_4dof_member_check <problem.bin> <result.bin>` dumps the flattened
//   problem in pose_graph_4dof_adapter_check.cc's layout, runs the member on the library, and dumps every keyframe's pose (7 floats), every
//   point's position and the SetPose counts.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "pose_graph_4dof_mock.h"
#include "Optimizer.h"

using namespace ORB_SLAM3;
std::mutex ORB_SLAM3::MapPoint::mGlobalMutex;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
template <class T> static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), n * sizeof(T)); }

static void rot_of(const PGQuat& q, double* R) {   // a unit quaternion's rotation matrix, row-major
  const double x = q.v[0], y = q.v[1], z = q.v[2], w = q.v[3];
  const double m[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                       2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
  std::memcpy(R, m, sizeof m);
}

struct Scene {
  PGMap map;
  std::vector<PGKeyFrame> kfs;
  std::vector<PGMapPoint> mps;
  std::map<PGKeyFrame*, PGSim3> NonCorrectedSim3, CorrectedSim3;
  std::map<PGKeyFrame*, std::set<PGKeyFrame*>> LoopConnections;
  static PGSim3 pose_sim3(const PGKeyFrame& K) {
    PGVec3 t;
    for (int c = 0; c < 3; ++c) t.v[c] = (double)K.mTcw.t[c];
    return PGSim3(PGQuat((double)K.mTcw.q[3], (double)K.mTcw.q[0], (double)K.mTcw.q[1], (double)K.mTcw.q[2]), t, 1.0);
  }
  Scene() : kfs(7), mps(5) {
    map.initKF = 1; map.inertial = true;
    Sophus::SE3f Tcb;   // the camera looks along the body's x: Rcb = [0 -1 0; 0 0 -1; 1 0 0]
    const float Rcb[9] = {0, -1, 0, 0, 0, -1, 1, 0, 0};
    for (int k = 0; k < 9; ++k) Tcb.R[k] = Rcb[k];
    Tcb.t[0] = 0.05f; Tcb.t[1] = -0.02f; Tcb.t[2] = 0.01f;
    for (int k = 0; k < 7; ++k) {
      PGKeyFrame& K = kfs[k];
      K.mnId = 2 * k + 1; K.mpMap = &map; K.mImuCalib.mTcb = Tcb;
      // the body yaws by 0.12 k rad about the vertical, with a little roll; Rcw = Rcb Rwb^T
      const double yaw = 0.12 * k, roll = 0.01 * k;
      const double Rwb[9] = {std::cos(yaw), -std::sin(yaw) * std::cos(roll), std::sin(yaw) * std::sin(roll), std::sin(yaw), std::cos(yaw) * std::cos(roll),
                             -std::cos(yaw) * std::sin(roll), 0, std::sin(roll), std::cos(roll)};
      const double twb[3] = {0.8 * k, 0.05 * k * k, 0.02 * k};
      double Rcw[9], tcw[3];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rcw[r * 3 + c] = Rcb[r * 3] * Rwb[c * 3] + Rcb[r * 3 + 1] * Rwb[c * 3 + 1] + Rcb[r * 3 + 2] * Rwb[c * 3 + 2];
      double tbw[3];
      for (int r = 0; r < 3; ++r) tbw[r] = -(Rwb[r] * twb[0] + Rwb[3 + r] * twb[1] + Rwb[6 + r] * twb[2]);
      for (int r = 0; r < 3; ++r) tcw[r] = Rcb[r * 3] * tbw[0] + Rcb[r * 3 + 1] * tbw[1] + Rcb[r * 3 + 2] * tbw[2] + Tcb.t[r];
      double q[4];
      morb_glue::matrix_to_quat(Rcw, q);
      for (int c = 0; c < 4; ++c) K.mTcw.q[c] = (float)q[c];
      for (int c = 0; c < 9; ++c) { K.mTcw.R[c] = (float)Rcw[c]; K.mRcw.m[c] = (float)Rcw[c]; K.mRwb.m[c] = (float)Rwb[c]; }
      for (int c = 0; c < 3; ++c) { K.mTcw.t[c] = (float)tcw[c]; K.mtcw.v[c] = (float)tcw[c]; K.mOwb.v[c] = (float)twb[c]; }
    }
    kfs[3].mbBad = true;
    const int order[7] = {0, 2, 1, 3, 4, 5, 6};   // GetAllKeyFrames() is not sorted by mnId
    for (int k : order) map.kfs.push_back(&kfs[k]);
    for (int k = 1; k < 7; ++k) { kfs[k].mPrevKF = &kfs[k - 1]; kfs[k - 1].mNextKF = &kfs[k]; }   // k4's mPrevKF is the bad k3
    auto cov = [&](int a, std::vector<std::pair<int, int>> l) { for (auto& kw : l) { kfs[a].covisibles.push_back(&kfs[kw.first]); kfs[a].weights[&kfs[kw.first]] = kw.second; } };
    cov(0, {{1, 300}});                                            // mNextKF (and of a larger mnId)
    cov(1, {{0, 300}});                                            // mPrevKF
    cov(2, {{1, 250}, {0, 150}, {4, 90}});                         // mPrevKF; an edge; below 100
    cov(4, {{2, 260}, {3, 240}, {5, 200}, {0, 130}, {1, 120}});    // an edge; mPrevKF (bad); mNextKF; a loop edge; an edge
    cov(5, {{4, 270}, {6, 220}, {2, 110}});                        // mPrevKF; mNextKF; its child
    cov(6, {{5, 280}, {2, 140}, {4, 130}});                        // mPrevKF; in sInsertedEdges; an edge
    kfs[5].children.insert(&kfs[2]);                                // (a parent of a larger mnId: what a map merge leaves)
    kfs[4].loopEdges.insert(&kfs[0]); kfs[0].loopEdges.insert(&kfs[4]);   // an old loop: an edge from k4 only
    kfs[6].weights[&kfs[1]] = 30; kfs[6].weights[&kfs[0]] = 40; kfs[5].weights[&kfs[1]] = 50; kfs[5].weights[&kfs[0]] = 100; kfs[5].weights[&kfs[3]] = 150;
    LoopConnections[&kfs[6]] = {&kfs[1], &kfs[0], &kfs[2]};   // (cur, loop) at weight 30: kept; k0 at 40: dropped; k2 at 140: kept
    LoopConnections[&kfs[5]] = {&kfs[1], &kfs[0], &kfs[3]};   // k1 at 50: dropped; k0 at 100: kept; k3 is bad: no edge
    // CorrectLoop's propagation: the current keyframe's corrected Sim3 (a yaw of the world, a translation, scale 1.03), and Sic * it for k5
    PGVec3 gt; gt.v[0] = 0.15; gt.v[1] = -0.05; gt.v[2] = 0.02;
    const PGSim3 Winv(PGQuat(std::cos(0.02), 0, 0, -std::sin(0.02)), gt, 1.0);
    const PGSim3 S6 = pose_sim3(kfs[6]), S5 = pose_sim3(kfs[5]);
    PGSim3 C6 = S6 * Winv;
    C6.s = 1.03;
    for (int c = 0; c < 3; ++c) C6.t.v[c] *= 1.03;
    NonCorrectedSim3[&kfs[6]] = S6; NonCorrectedSim3[&kfs[5]] = S5;
    CorrectedSim3[&kfs[6]] = C6; CorrectedSim3[&kfs[5]] = (S5 * S6.inverse()) * C6;
    for (int j = 0; j < 5; ++j) { mps[j].mnId = j; mps[j].mpMap = &map; mps[j].mWorldPos = Eigen::Vector3f(1.f + j, 0.5f * j, 4.f - 0.3f * j); map.mps.push_back(&mps[j]); }
    mps[0].ref = &kfs[2];
    mps[1].ref = &kfs[5];
    mps[2].ref = &kfs[1]; mps[2].mbBad = true;
    mps[3].ref = &kfs[6];
    mps[4].ref = &kfs[3];   // its reference keyframe is bad: no vertex, the point keeps its position
  }
};

#ifdef PG4_STUB_ENTRY
static int g_calls = 0, g_bad = 0;
struct Expect { std::vector<double> kfPose, kfBody, kfScw, eTij; std::vector<uint8_t> kfFixed; std::vector<int> eI, eJ, mpRef; std::vector<float> mpPos, Tcb12; } g_expect;
static bool close_to(const std::vector<double>& v, const double* p, size_t n) {
  if (v.size() != n) return false;
  for (size_t i = 0; i < n; ++i) if (!(std::fabs(v[i] - p[i]) <= 1e-12 * (1 + std::fabs(v[i])))) return false;
  return true;
}
extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
int morb_optimizer_create(morb_optimizer** out, int) { static int token; *out = reinterpret_cast<morb_optimizer*>(&token); return MORB_OK; }
int morb_optimizer_set_exact_order(morb_optimizer*, int) { return MORB_OK; }
const char* morb_last_error(void) { return "stub"; }
int morb_optimize_essential_graph_4dof(morb_optimizer*, int nKF, double* kfPose, const double* kfBody, const uint8_t* kfFixed, const float* Tcb12, int nE,
                                       const int* eI, const int* eJ, const double* eTij, int nMP, float* mpPos, const int* mpRef, const double* kfScw,
                                       int* stats4, double* chi2) {
  ++g_calls;
  const Expect& x = g_expect;
  auto same = [](const auto& v, const auto* p, size_t n) { return v.size() == n && (n == 0 || std::memcmp(v.data(), p, n * sizeof(v[0])) == 0); };
  if (!same(x.kfFixed, kfFixed, nKF)) { ++g_bad; std::printf("fixed flags differ\n"); }
  if (!same(x.Tcb12, Tcb12, 12)) { ++g_bad; std::printf("calibration differs\n"); }
  if (!close_to(x.kfPose, kfPose, (size_t)nKF * 12)) { ++g_bad; std::printf("poses differ\n"); }
  if (!close_to(x.kfBody, kfBody, (size_t)nKF * 12)) { ++g_bad; std::printf("body states differ\n"); }
  if (!kfScw || !close_to(x.kfScw, kfScw, (size_t)nKF * 8)) { ++g_bad; std::printf("vScw differs\n"); }
  if (!same(x.eI, eI, nE) || !same(x.eJ, eJ, nE)) {
    ++g_bad; std::printf("edge list differs:");
    for (int e = 0; e < nE; ++e) std::printf(" (%d,%d)", eI[e], eJ[e]);
    std::printf("\n");
  } else if (!close_to(x.eTij, eTij, (size_t)nE * 12)) { ++g_bad; std::printf("measurements differ\n"); }
  if (!same(x.mpRef, mpRef, nMP) || !same(x.mpPos, mpPos, (size_t)nMP * 3)) { ++g_bad; std::printf("points differ\n"); }
  for (int v = 0; v < nKF; ++v) {   // canned: a yaw of 0.1 (v + 1) rad, translation 10 + v ..
    double* P = kfPose + 12 * v;
    const double a = 0.1 * (v + 1);
    const double R[9] = {std::cos(a), -std::sin(a), 0, std::sin(a), std::cos(a), 0, 0, 0, 1};
    std::memcpy(P, R, sizeof R);
    P[9] = 10.0 + v; P[10] = 20.0 + v; P[11] = 30.0 + v;
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
  PGMap* pLoopMap = &sc.map;
  PGKeyFrame *mpLoopMatchedKF = &sc.kfs[1], *mpCurrentKF = &sc.kfs[6];
  auto& NonCorrectedSim3 = sc.NonCorrectedSim3; auto& CorrectedSim3 = sc.CorrectedSim3; auto& LoopConnections = sc.LoopConnections;
#ifdef PG4_STUB_ENTRY
  (void)argc; (void)argv;
  {   // the expectation, written out by hand.  Vertices in ascending mnId: k0 k1 k2 k4 k5 k6 -> 0 .. 5
    Expect& x = g_expect;
    PGKeyFrame* byRow[6] = {&sc.kfs[0], &sc.kfs[1], &sc.kfs[2], &sc.kfs[4], &sc.kfs[5], &sc.kfs[6]};
    std::vector<PGSim3> V(6), N(6);   // vScw, and what a normal edge takes: NonCorrectedSim3's entry or vScw
    for (int r = 0; r < 6; ++r) { V[r] = r >= 4 ? sc.CorrectedSim3[byRow[r]] : Scene::pose_sim3(*byRow[r]); N[r] = r >= 4 ? sc.NonCorrectedSim3[byRow[r]] : V[r]; }
    x.kfFixed = {0, 1, 0, 0, 0, 0};   // pLoopKF
    const float Tcb12[12] = {0, -1, 0, 0, 0, -1, 1, 0, 0, 0.05f, -0.02f, 0.01f};
    x.Tcb12.assign(Tcb12, Tcb12 + 12);
    for (int r = 0; r < 6; ++r) {
      double P[12], B[12], s8[8] = {V[r].r.v[0], V[r].r.v[1], V[r].r.v[2], V[r].r.v[3], V[r].t.v[0], V[r].t.v[1], V[r].t.v[2], V[r].s};
      if (r < 4) {   // the float members
        for (int c = 0; c < 9; ++c) { P[c] = (double)byRow[r]->mRcw.m[c]; B[c] = (double)byRow[r]->mRwb.m[c]; }
        for (int c = 0; c < 3; ++c) { P[9 + c] = (double)byRow[r]->mtcw.v[c]; B[9 + c] = (double)byRow[r]->mOwb.v[c]; }
      } else {       // Swc = CorrectedSim3^-1: Rwb = Rwc Rcb, twb = Rwc tcb + twc, Rcw = Rwc^T, tcw = -Rcw twc
        const PGSim3 Swc = V[r].inverse();
        double Rwc[9];
        rot_of(Swc.r, Rwc);
        for (int a = 0; a < 3; ++a) {
          B[9 + a] = Rwc[a * 3] * (double)Tcb12[9] + Rwc[a * 3 + 1] * (double)Tcb12[10] + Rwc[a * 3 + 2] * (double)Tcb12[11] + Swc.t.v[a];
          for (int c = 0; c < 3; ++c) {
            B[a * 3 + c] = Rwc[a * 3] * Tcb12[c] + Rwc[a * 3 + 1] * Tcb12[3 + c] + Rwc[a * 3 + 2] * Tcb12[6 + c];
            P[a * 3 + c] = Rwc[c * 3 + a];
          }
        }
        for (int a = 0; a < 3; ++a) P[9 + a] = -(P[a * 3] * Swc.t.v[0] + P[a * 3 + 1] * Swc.t.v[1] + P[a * 3 + 2] * Swc.t.v[2]);
      }
      x.kfPose.insert(x.kfPose.end(), P, P + 12); x.kfBody.insert(x.kfBody.end(), B, B + 12); x.kfScw.insert(x.kfScw.end(), s8, s8 + 8);
    }
    REQUIRE(V[5].s == 1.03 && std::fabs(V[4].s - 1.03) < 1e-12);
    struct E { int i, j; bool loop; };
    const E edges[] = {{4, 0, true}, {5, 1, true}, {5, 2, true},                 // LoopConnections: k5 -> k0; k6 -> k1 (the pair), k6 -> k2
                       {2, 1, false}, {2, 0, false},                             // k2: mPrevKF, covisible k0
                       {1, 0, false},                                            // k1: mPrevKF
                       {3, 0, false}, {3, 2, false}, {3, 1, false},              // k4: old loop edge to k0, covisibles k2 and k1 (its mPrevKF is bad)
                       {4, 3, false},                                            // k5: mPrevKF
                       {5, 4, false}, {5, 3, false}};                            // k6: mPrevKF, covisible k4
    for (const E& e : edges) {
      x.eI.push_back(e.i); x.eJ.push_back(e.j);
      const PGSim3 M = e.loop ? V[e.i] * V[e.j].inverse() : N[e.i] * N[e.j].inverse();
      double T[12];
      rot_of(M.r, T);
      for (int c = 0; c < 3; ++c) T[9 + c] = M.t.v[c];
      x.eTij.insert(x.eTij.end(), T, T + 12);
    }
    x.mpRef = {2, 4, -1, 5, -1};
    for (int j = 0; j < 5; ++j) for (int c = 0; c < 3; ++c) x.mpPos.push_back(j == 2 ? 0.f : sc.mps[j].mWorldPos.v[c]);
  }
  Optimizer::OptimizeEssentialGraph4DoF(pLoopMap, mpLoopMatchedKF,
                                          mpCurrentKF, NonCorrectedSim3,
                                          CorrectedSim3, LoopConnections);
  REQUIRE(g_calls == 1 && g_bad == 0);
  const int rowOf[7] = {0, 1, 2, -1, 3, 4, 5};
  for (int k = 0; k < 7; ++k) {   // SetPose on every keyframe that has a vertex: the unit quaternion of Rcw and tcw, as floats
    REQUIRE(sc.kfs[k].nSetPose == (k == 3 ? 0 : 1));
    if (k == 3) continue;
    const int v = rowOf[k];
    const double a = 0.1 * (v + 1);
    REQUIRE(std::fabs(sc.kfs[k].mTcw.q[2] - std::sin(a / 2)) < 1e-6 && std::fabs(sc.kfs[k].mTcw.q[3] - std::cos(a / 2)) < 1e-6 && sc.kfs[k].mTcw.q[0] == 0.f);
    REQUIRE(sc.kfs[k].mTcw.t[0] == (float)(10.0 + v) && sc.kfs[k].mTcw.t[2] == (float)(30.0 + v));
  }
  for (int j = 0; j < 5; ++j) {
    REQUIRE(sc.mps[j].nSetPos == ((j == 2 || j == 4) ? 0 : 1) && sc.mps[j].nUpdates == (j == 2 ? 0 : 1));
    if (j != 2 && j != 4) REQUIRE(sc.mps[j].mWorldPos.v[1] == 200.f + 3 * j + 1);
  }
  REQUIRE(sc.map.changes == 1);
  std::printf("pose graph 4dof member ok\n");
  return 0;
#else
  if (argc < 3) { std::printf("usage: %s problem.bin result.bin\n", argv[0]); return 2; }
  PoseGraph4DoFFlat f;
  morb_glue::flatten_pose_graph_4dof(pLoopMap, mpLoopMatchedKF, mpCurrentKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, f);
  {
    std::ofstream out(argv[1], std::ios::binary);
    const int hd[3] = {(int)f.kfFixed.size(), (int)f.eI.size(), (int)f.mpRef.size()};
    wr(out, hd, 3); wr(out, f.kfPose.data(), f.kfPose.size()); wr(out, f.kfBody.data(), f.kfBody.size()); wr(out, f.kfFixed.data(), f.kfFixed.size());
    wr(out, f.Tcb12, 12); wr(out, f.eI.data(), f.eI.size()); wr(out, f.eJ.data(), f.eJ.size()); wr(out, f.eTij.data(), f.eTij.size());
    wr(out, f.mpPos.data(), f.mpPos.size()); wr(out, f.mpRef.data(), f.mpRef.size()); wr(out, f.kfScw.data(), f.kfScw.size());
  }
  Optimizer::OptimizeEssentialGraph4DoF(pLoopMap, mpLoopMatchedKF,
                                          mpCurrentKF, NonCorrectedSim3,
                                          CorrectedSim3, LoopConnections);
  std::ofstream out(argv[2], std::ios::binary);
  for (int k = 0; k < 7; ++k) { wr(out, sc.kfs[k].mTcw.q, 4); wr(out, sc.kfs[k].mTcw.t, 3); }
  for (int j = 0; j < 5; ++j) wr(out, sc.mps[j].mWorldPos.v, 3);
  for (int k = 0; k < 7; ++k) wr(out, &sc.kfs[k].nSetPose, 1);
  return out ? 0 : 1;
#endif
}
