// Nothing of one adapter call may outlive it: Tracking builds a stack ORBmatcher per search (SearchLocalPoints), destroys it — and its
// stream with it — and calls Optimizer::PoseOptimization on the same thread.  Here the matcher call even throws after it has queued its
// uploads (70000 features: morb_search_by_projection_last_batch refuses cap > 65535 with MORB_ERR_INVALID), and the optimizer handle
// exists before the matcher, so that no stream is created between the matcher's destruction and the next call (a freed stream's address
// cannot be handed out again).  Inputs written by tests/test_adapter_gpu.py, which compares the dumps with the CPU oracle.
//   adapter_stream_lifetime_check <dir>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/morb/ORBmatcher.h"
#include "../../include/morb/Optimizer.h"

static std::string g_dir;
template <typename T>
static std::vector<T> load(const char* name) {
  std::ifstream f(g_dir + "/" + name + ".bin", std::ios::binary | std::ios::ate);
  if (!f) { std::fprintf(stderr, "missing %s\n", name); std::exit(3); }
  const size_t bytes = (size_t)f.tellg();
  std::vector<T> v(bytes / sizeof(T));
  f.seekg(0); f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)bytes);
  return v;
}
template <typename T>
static void dump(const std::string& name, const T* p, size_t n) {
  std::ofstream f(g_dir + "/out_" + name + ".bin", std::ios::binary);
  f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T)));
}

int main(int argc, char** argv) {
  using namespace ORB_SLAM3;
  if (argc < 2) return 2;
  g_dir = argv[1];
  const auto has = load<uint8_t>("po_has"); const auto obs = load<float>("po_obs"); const auto inv = load<float>("po_inv"); const auto Xw = load<float>("po_xw");
  const auto cam = load<float>("po_cam"); const auto pose = load<float>("po_pose");
  auto pose_optimization = [&](const std::string& tag) {
    PoseOptimizationView f;
    f.N = (int)has.size(); f.hasMapPoint = has.data(); f.obs = obs.data(); f.invSigma2 = inv.data(); f.worldPos = Xw.data();
    f.fx = cam[0]; f.fy = cam[1]; f.cx = cam[2]; f.cy = cam[3]; f.mbf = cam[4];
    for (int i = 0; i < 7; ++i) f.pose[i] = pose[i];
    const int nin = Optimizer::PoseOptimization(f);
    dump(tag + "_nin", &nin, 1); dump(tag + "_pose", f.pose, 7); dump(tag + "_outlier", f.mvbOutlier.data(), f.mvbOutlier.size());
  };
  const auto kps = load<morb_keypoint>("bow_kps"); const auto dKF = load<uint8_t>("bow_kf_desc"); const auto dF = load<uint8_t>("bow_f_desc");
  const auto nodeKF = load<int>("bow_kf_node"); const auto nodeF = load<int>("bow_f_node"); const auto hasKF = load<uint8_t>("bow_kf_hasmp");
  auto search_by_bow = [&](const std::string& tag) {
    KeyFrameView KF; KF.N = (int)kps.size(); KF.mvKeysUn = kps.data(); KF.mDescriptors = dKF.data(); KF.featNode = nodeKF.data(); KF.hasMapPoint = hasKF.data();
    FrameView F; F.N = (int)kps.size(); F.mvKeysUn = kps.data(); F.mDescriptors = dF.data(); F.featNode = nodeF.data();
    ORBmatcher matcher(0.7f, true);
    std::vector<int> match;
    const int n = matcher.SearchByBoW(KF, F, match);
    dump(tag + "_n", &n, 1); dump(tag + "_match", match.data(), match.size());
  };

  pose_optimization("before");   // the undisturbed run; creates the optimizer handle and its stream
  search_by_bow("bow_before");
  {
    const int N = 70000;
    const std::vector<morb_keypoint> big(N, kps[0]);
    const std::vector<uint8_t> bigDesc((size_t)N * 32, 0x5A);
    FrameView Cur, Last;
    Cur.N = Last.N = N; Cur.mvKeysUn = Last.mvKeysUn = big.data(); Cur.mDescriptors = Last.mDescriptors = bigDesc.data();
    ORBmatcher matcher(0.9f, true);
    std::vector<int> match;
    bool refused = false;
    try { matcher.SearchByProjection(Cur, Last, match, 7.f, false); }
    catch (const std::runtime_error& e) { refused = true; std::printf("refused as expected: %s\n", e.what()); }
    if (!refused) { std::fprintf(stderr, "the oversized search did not throw\n"); return 4; }
  }   // ~ORBmatcher: the stream the failed call queued its uploads on is gone
  pose_optimization("after");
  search_by_bow("bow_after");
  std::printf("stream lifetime ok\n");
  return 0;
}
