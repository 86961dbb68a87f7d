// Drop-in adapter: ORB_SLAM3::TwoViewReconstruction (reference include/TwoViewReconstruction.h, src/TwoViewReconstruction.cc) over
// morb_two_view_reconstruction_batch on the Optimizer's kTracking handle: what Pinhole::ReconstructWithTwoViews
// (src/CameraModels/Pinhole.cpp:85-98) constructs once and calls for every frame of Tracking::MonocularInitialization
// (src/Tracking.cc:2314-2330).  The members are templates on the caller's matrix / keypoint / SE3 / point types, so this header
// includes none of them: K is anything with operator()(r, c) (Eigen::Matrix3f), a keypoint anything with pt.x / pt.y, T21 a Sophus::SE3f,
// a point anything built from (x, y, z) (cv::Point3f).
//   * Reconstruct draws 8 * iterations values from rand() per call, in the reference's order, after srand(0) once per process
//     (DUtils::Random::SeedRandOnce(0), :80): the reference's stream is followed call after call.  The handle is created BEFORE the
//     seeding, so whatever the HIP runtime does when it starts cannot move the stream.  The exception: a call with fewer than eight
//     matches draws nothing (the reference's draws are undefined there: RandomInt(0, -1) on an empty vector).
//   * vP3D is assigned on both paths.  The reference's ReconstructH (:712-718) returns true without assigning it (upstream ORB-SLAM3
//     assigns bestP3D there); a caller that reads vP3D after a homography initialisation gets the points here.
//   * fewer than eight matches: false (the reference's behaviour is undefined).
//   * the keypoints are the UNDISTORTED ones; KannalaBrandt8::ReconstructWithTwoViews undistorts with cv::fisheye::undistortPoints
//     first, which is the caller's to do.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#include "Optimizer.h"
#include "two_view_math.h"

namespace ORB_SLAM3 {

// the view-taking form: plain arrays in, plain arrays out
struct TwoViewView {
  int n1 = 0, n2 = 0;
  const float *kp1 = nullptr, *kp2 = nullptr;   // [n][2] undistorted keypoint positions
  const int* matches12 = nullptr;               // [n1] vMatches12
  float T21[12] = {0};                          // out: R21 row-major, t21 (zero unless true is returned)
  std::vector<float> P3D;                       // out: [n1][3]
  std::vector<uint8_t> triangulated;            // out: [n1]
  int stats[morbtv::TV_STATS_LEN] = {0};        // out: morbtv::TwoViewStat
  float fstats[morbtv::TV_FSTATS_LEN] = {0};    // out: morbtv::TwoViewFStat
};

class TwoViewReconstruction {
 public:
  // TwoViewReconstruction(const Eigen::Matrix3f& k, float sigma = 1.0, int iterations = 200)  (:32-39)
  template <class Mat3>
  explicit TwoViewReconstruction(const Mat3& k, float sigma = 1.0, int iterations = 200, int device = 0)
      : sigma_(sigma), iterations_(iterations), device_(device) {
    K4_[0] = k(0, 0); K4_[1] = k(1, 1); K4_[2] = k(0, 2); K4_[3] = k(1, 2);
  }

  // bool Reconstruct(const vector<cv::KeyPoint>& vKeys1, const vector<cv::KeyPoint>& vKeys2, const vector<int>& vMatches12,
  //                  Sophus::SE3f& T21, vector<cv::Point3f>& vP3D, vector<bool>& vbTriangulated)  (:41-130)
  template <class KP, class SE3, class P3>
  bool Reconstruct(const std::vector<KP>& vKeys1, const std::vector<KP>& vKeys2, const std::vector<int>& vMatches12, SE3& T21,
                   std::vector<P3>& vP3D, std::vector<bool>& vbTriangulated) {
    TwoViewView v;
    v.n1 = (int)vKeys1.size(); v.n2 = (int)vKeys2.size();
    std::vector<float> a((size_t)v.n1 * 2), b((size_t)v.n2 * 2);
    for (int i = 0; i < v.n1; ++i) { a[(size_t)i * 2] = vKeys1[i].pt.x; a[(size_t)i * 2 + 1] = vKeys1[i].pt.y; }
    for (int i = 0; i < v.n2; ++i) { b[(size_t)i * 2] = vKeys2[i].pt.x; b[(size_t)i * 2 + 1] = vKeys2[i].pt.y; }
    std::vector<int> m(v.n1, -1);   // :58 reads vMatches12.size() entries; an entry beyond mvKeys1 would be read out of bounds there
    for (int i = 0; i < v.n1 && i < (int)vMatches12.size(); ++i) m[i] = vMatches12[i];
    v.kp1 = a.data(); v.kp2 = b.data(); v.matches12 = m.data();
    if (!Reconstruct(v)) return false;
    typename std::decay<decltype(std::declval<SE3>().rotationMatrix())>::type R;
    typename SE3::Point t;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) R(r, c) = v.T21[r * 3 + c];
      t(r) = v.T21[9 + r];
    }
    T21 = SE3(R, t);
    vP3D.clear();
    vbTriangulated.assign(v.n1, false);
    for (int i = 0; i < v.n1; ++i) {
      vP3D.push_back(P3(v.P3D[(size_t)i * 3], v.P3D[(size_t)i * 3 + 1], v.P3D[(size_t)i * 3 + 2]));
      vbTriangulated[i] = v.triangulated[i] != 0;
    }
    return true;
  }

  bool Reconstruct(TwoViewView& v) {
    const int n1 = v.n1, n2 = v.n2, cap = std::max(std::max(n1, n2), 1);
    Optimizer::Slot& o = Optimizer::slot(device_, Optimizer::kTracking);   // the device starts here, before the seeding
    SeedRandOnce();
    const int nrand = morbtv::TV_SET * (iterations_ > 0 ? iterations_ : 0);
    std::vector<int> rnd((size_t)std::max(nrand, 1), 0);
    int N = 0;
    for (int i = 0; i < n1; ++i) N += v.matches12[i] >= 0 && v.matches12[i] < n2;
    if (N >= morbtv::TV_SET)   // the reference draws nothing it could define below eight matches
      for (int k = 0; k < nrand; ++k) rnd[k] = std::rand();
    std::vector<morb_keypoint> kps((size_t)2 * cap);
    for (int i = 0; i < n1; ++i) { kps[i] = morb_keypoint{}; kps[i].x = v.kp1[(size_t)i * 2]; kps[i].y = v.kp1[(size_t)i * 2 + 1]; }
    for (int i = 0; i < n2; ++i) { kps[(size_t)cap + i] = morb_keypoint{}; kps[(size_t)cap + i].x = v.kp2[(size_t)i * 2]; kps[(size_t)cap + i].y = v.kp2[(size_t)i * 2 + 1]; }
    std::vector<int> m(cap, -1);
    for (int i = 0; i < n1; ++i) m[i] = v.matches12[i];
    const int img[2] = {0, 1}, count[2] = {n1, n2};
    v.P3D.assign((size_t)cap * 3, 0.f);
    v.triangulated.assign(cap, 0);
    int ok = 0;
    {
      std::lock_guard<std::mutex> lock(o.mu);
      Optimizer::Call c(device_, morb_optimizer_stream(o.h));
      const int *d_img = c.in(img, 2), *d_count = c.in(count, 2), *d_m = c.in(m.data(), cap), *d_rand = c.in(rnd.data(), rnd.size());
      const morb_keypoint* d_kps = c.in(kps.data(), kps.size());
      const float *d_K4 = c.in(K4_, 4), *d_sigma = c.in(&sigma_, 1);
      int *d_ok = c.out<int>(1), *d_stats = c.out<int>(morbtv::TV_STATS_LEN);
      float *d_T21 = c.out<float>(12), *d_P3D = c.out<float>((size_t)cap * 3), *d_fstats = c.out<float>(morbtv::TV_FSTATS_LEN);
      uint8_t* d_tri = c.out<uint8_t>(cap);
      Optimizer::check(morb_two_view_reconstruction_batch(o.h, 1, cap, d_img, d_img + 1, d_count, d_kps, d_m, d_K4, d_sigma, iterations_, d_rand,
                                                          (int)rnd.size(), d_ok, d_T21, d_P3D, d_tri, d_stats, d_fstats, nullptr, nullptr, nullptr,
                                                          nullptr));
      c.wait();
      c.fetch(d_ok, &ok, 1);
      c.fetch(d_T21, v.T21, 12);
      c.fetch(d_P3D, v.P3D.data(), (size_t)cap * 3);
      c.fetch(d_tri, v.triangulated.data(), cap);
      c.fetch(d_stats, v.stats, morbtv::TV_STATS_LEN);
      c.fetch(d_fstats, v.fstats, morbtv::TV_FSTATS_LEN);
    }
    v.P3D.resize((size_t)n1 * 3);
    v.triangulated.resize(n1);
    return ok != 0;
  }

  // DUtils::Random::SeedRandOnce(0): srand(0) the first time any TwoViewReconstruction of the process reconstructs
  static void SeedRandOnce() {
    static std::once_flag once;
    std::call_once(once, [] { std::srand(0); });
  }

 private:
  float K4_[4] = {0, 0, 0, 0};
  float sigma_ = 1.f;
  int iterations_ = 200, device_ = 0;
};

}  // namespace ORB_SLAM3
