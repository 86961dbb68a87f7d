// Drop-in adapter: ORB_SLAM3::Sim3Solver (reference include/Sim3Solver.h, src/Sim3Solver.cc) over morb_sim3_solver_batch on the
// Optimizer's kLoopClosing handle.  The reference's constructor is a member template on its KeyFrame / MapPoint types (as in
// Optimizer_reference.h), so this header includes none of them; the Eigen results come back as small matrices that convert to any
// type with operator()(r, c) / operator()(i) (Eigen::Matrix4f, Matrix3f, Vector3f).
//   * Samples are drawn with rand() in the reference's order, three per iteration, once per iterate call for that call's budget
//     (min(nIterations, remaining iterations); none when N < minInliers).  The one divergence: the reference stops drawing at the
//     iteration that converges, this adapter has drawn the whole call's values by then.  rand() is process-global and shared by the
//     Tracking and LoopClosing threads, so its position is not deterministic in the reference either.
//   * iterate(.., bConverge) returns identity where the reference returns its uninitialised bestSim3 (no iteration of the call
//     reached the best count).
//   * No console output (the reference prints "Empty Keyframe" / "Not Empty" from its constructor).
#pragma once
#include <cstdlib>
#include <mutex>
#include <tuple>
#include <vector>

#include "Optimizer.h"
#include "sim3_solver_math.h"

namespace ORB_SLAM3 {

namespace morb_s3 {
template <int R, int C>
struct SmallMat {   // row-major float matrix that converts to the caller's Eigen type
  float m[R * C];
  float operator()(int r, int c) const { return m[r * C + c]; }
  float operator()(int i) const { return m[i]; }
  template <class M>
  operator M() const {
    M out;
    assign(out, 0);
    return out;
  }

 private:
  template <class M>
  auto assign(M& out, int) const -> decltype(out(0, 0) = 0.f, void()) {
    for (int r = 0; r < R; ++r)
      for (int c = 0; c < C; ++c) out(r, c) = m[r * C + c];
  }
  template <class M>
  void assign(M& out, long) const {
    for (int i = 0; i < R * C; ++i) out(i) = m[i];
  }
};
}  // namespace morb_s3

// One problem as morb_sim3_solver_batch takes it (include/morb_hip.h): per KF1 feature entry bits, world points and sigma2 of both
// keypoints; the per-problem parameters.  The view constructor honours params.probability / minInliers / maxIterations (defaults:
// SetRansacParameters' 0.99 / 6 / 300); the reference-signature constructor resets them to those defaults, as the reference does.
struct Sim3SolverView {
  int N1 = 0;                              // mN1 = vpMatched12.size()
  std::vector<uint8_t> entry;              // [N1]
  std::vector<float> Xw1, Xw2;             // [N1][3]
  std::vector<float> sigma2_1, sigma2_2;   // [N1]
  morb_sim3_solver_params params{};
  Sim3SolverView() {
    params.probability = 0.99;
    params.minInliers = 6;
    params.maxIterations = 300;
  }
};

class Sim3Solver {
 public:
  using Mat4 = morb_s3::SmallMat<4, 4>;
  using Mat3 = morb_s3::SmallMat<3, 3>;
  using Vec3 = morb_s3::SmallMat<3, 1>;

  // Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const vector<MapPoint*>& vpMatched12, const bool bFixScale = true,
  //            const vector<KeyFrame*> vpKeyFrameMatchedMP = vector<KeyFrame*>())  Sim3Solver.cc:34-120
  template <class KF, class MP>
  Sim3Solver(KF* pKF1, KF* pKF2, const std::vector<MP*>& vpMatched12, const bool bFixScale = true,
             std::vector<KF*> vpKeyFrameMatchedMP = std::vector<KF*>(), int device = 0)
      : device_(device) {
    Sim3SolverView& v = view_;
    const int n = (int)vpMatched12.size();
    const bool bDifferentKFs = vpKeyFrameMatchedMP.empty();
    const std::vector<MP*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    v.N1 = n;
    v.entry.assign(n, 0);
    v.Xw1.assign((size_t)n * 3, 0.f); v.Xw2.assign((size_t)n * 3, 0.f);
    v.sigma2_1.assign(n, 0.f); v.sigma2_2.assign(n, 0.f);
    // a rig keyframe's mvKeysUn holds its left keypoints only: feature i's own row
    auto key_of = [](KF* pKF, int i) -> decltype(pKF->mvKeysUn[0]) {
      return (pKF->NLeft != -1 && i >= pKF->NLeft) ? pKF->mvKeysRight[i - pKF->NLeft] : pKF->mvKeysUn[i];
    };
    for (int i1 = 0; i1 < n; ++i1) {
      MP* pMP2 = vpMatched12[i1];
      if (!pMP2) continue;
      uint8_t e = 1;
      MP* pMP1 = vpKeyFrameMP1[i1];
      if (pMP1) {
        e |= 2;
        if (pMP1->isBad()) e |= 4;
      }
      if (pMP2->isBad()) e |= 8;
      v.entry[i1] = e;
      if (e != 3) continue;   // the constructor reads nothing more of this match
      KF* pKFm = bDifferentKFs ? pKF2 : vpKeyFrameMatchedMP[i1];
      const int indexKF1 = std::get<0>(pMP1->GetIndexInKeyFrame(pKF1));
      const int indexKF2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKFm));
      if (indexKF1 < 0) e |= 16;
      if (indexKF2 < 0) e |= 32;
      v.entry[i1] = e;
      if (e != 3) continue;
      v.sigma2_1[i1] = pKF1->mvLevelSigma2[key_of(pKF1, indexKF1).octave];
      v.sigma2_2[i1] = pKFm->mvLevelSigma2[key_of(pKFm, indexKF2).octave];
      const auto X1 = pMP1->GetWorldPos();
      const auto X2 = pMP2->GetWorldPos();
      for (int k = 0; k < 3; ++k) { v.Xw1[(size_t)i1 * 3 + k] = X1(k); v.Xw2[(size_t)i1 * 3 + k] = X2(k); }
    }
    auto pose12 = [](KF* pKF, float* T) {
      const auto Tcw = pKF->GetPose();
      const auto R = Tcw.rotationMatrix();
      const auto t = Tcw.translation();
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T[r * 3 + c] = R(r, c);
      for (int k = 0; k < 3; ++k) T[9 + k] = t(k);
    };
    pose12(pKF1, v.params.T1w);
    pose12(pKF2, v.params.T2w);
    auto cam9 = [](KF* pKF, float* c) {
      morb_glue::cam8(pKF->mpCamera, c + 1);
      c[0] = pKF->mpCamera->size() >= 8 ? 1.f : 0.f;
    };
    cam9(pKF1, v.params.cam1);
    cam9(pKF2, v.params.cam2);
    v.params.fixScale = bFixScale ? 1 : 0;
    v.params.n = n;
    init(0.99, 6, 300);   // the constructor's SetRansacParameters() with its defaults (:117)
  }
  // the view form: the view's RANSAC parameters hold until SetRansacParameters is called
  explicit Sim3Solver(const Sim3SolverView& v, int device = 0) : view_(v), device_(device) {
    init(v.params.probability, v.params.minInliers, v.params.maxIterations);
  }

  // SetRansacParameters (:122-146): also restarts the iterations, as the reference does
  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    view_.params.probability = probability;
    view_.params.minInliers = minInliers;
    view_.params.maxIterations = maxIterations;
    budget_ = morbs3::sim3s_budget(N_, minInliers, probability, maxIterations);
    rand_.assign((size_t)3 * budget_, 0);
    state_.iterations = 0;
  }

  Mat4 find(std::vector<bool>& vbInliers12, int& nInliers) {
    bool bFlag, bConverge;
    const Mat4 T = run(view_.params.maxIterations, bFlag, vbInliers12, nInliers, bConverge);
    return bConverge ? T : identity();
  }
  Mat4 iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    bool bConverge;
    const Mat4 T = run(nIterations, bNoMore, vbInliers, nInliers, bConverge);
    return bConverge ? T : identity();
  }
  Mat4 iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge) {
    return run(nIterations, bNoMore, vbInliers, nInliers, bConverge);
  }

  Mat4 GetEstimatedTransformation() const { return make<4, 4>(state_.bestT12); }
  Mat3 GetEstimatedRotation() const { return make<3, 3>(state_.bestR); }
  Vec3 GetEstimatedTranslation() const { return make<3, 1>(state_.bestt); }
  float GetEstimatedScale() const { return state_.bestScale; }
  const morb_sim3_solver_state& state() const { return state_; }

 private:
  template <int R, int C>
  static morb_s3::SmallMat<R, C> make(const float* p) {
    morb_s3::SmallMat<R, C> m;
    for (int i = 0; i < R * C; ++i) m.m[i] = p[i];
    return m;
  }
  static Mat4 identity() {
    Mat4 m;
    for (int i = 0; i < 16; ++i) m.m[i] = (i % 5 == 0) ? 1.f : 0.f;
    return m;
  }
  void init(double probability, int minInliers, int maxIterations) {
    N_ = 0;
    for (int i = 0; i < view_.N1; ++i) N_ += view_.entry[i] == 3;
    state_ = morb_sim3_solver_state{};
    SetRansacParameters(probability, minInliers, maxIterations);
  }
  Mat4 run(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge) {
    const morb_sim3_solver_params& P = view_.params;
    const int n = view_.N1;
    // the rand() values this call's iterations draw, in the reference's order
    int its = 0;
    if (N_ >= P.minInliers && N_ >= 3) {
      its = budget_ - state_.iterations;
      if (nIterations < its) its = nIterations > 0 ? nIterations : 0;
    }
    for (int k = 0; k < 3 * its; ++k) rand_[(size_t)3 * state_.iterations + k] = std::rand();
    std::vector<uint8_t> mask(n > 0 ? n : 1, 0);
    if (n > 0) {
      Optimizer::Slot& o = Optimizer::slot(device_, Optimizer::kLoopClosing);
      std::lock_guard<std::mutex> lock(o.mu);
      Optimizer::Call c(device_, morb_optimizer_stream(o.h));
      const int randCap = (int)rand_.size();
      const morb_sim3_solver_params* d_params = c.in(&P, 1);
      const uint8_t* d_entry = c.in(view_.entry.data(), n);
      const float *d_Xw1 = c.in(view_.Xw1.data(), (size_t)n * 3), *d_Xw2 = c.in(view_.Xw2.data(), (size_t)n * 3);
      const float *d_sigma2_1 = c.in(view_.sigma2_1.data(), n), *d_sigma2_2 = c.in(view_.sigma2_2.data(), n);
      const int* d_rand = randCap > 0 ? c.in(rand_.data(), rand_.size()) : nullptr;
      morb_sim3_solver_state* d_state = c.in(&state_, 1);
      uint8_t* d_inliers = c.out<uint8_t>(n);
      Optimizer::check(morb_sim3_solver_batch(o.h, 1, n, d_params, d_entry, d_Xw1, d_Xw2, d_sigma2_1, d_sigma2_2, nIterations, d_rand, randCap, d_state,
                                              d_inliers, nullptr, 0, nullptr));
      c.wait();
      c.fetch(d_state, &state_, 1);
      c.fetch(d_inliers, mask.data(), n);
    } else {   // mN1 = 0: N = 0 < minInliers
      state_.converged = 0; state_.noMore = 1; state_.nInliers = 0;
      for (int i = 0; i < 16; ++i) state_.sim3[i] = (i % 5 == 0) ? 1.f : 0.f;
    }
    vbInliers.assign(n, false);
    for (int i = 0; i < n; ++i) vbInliers[i] = mask[i] != 0;
    bNoMore = state_.noMore != 0;
    bConverge = state_.converged != 0;
    nInliers = state_.nInliers;
    return make<4, 4>(state_.sim3);
  }

  Sim3SolverView view_;
  int device_ = 0;
  int N_ = 0, budget_ = 1;
  std::vector<int> rand_;
  morb_sim3_solver_state state_{};
};

}  // namespace ORB_SLAM3
