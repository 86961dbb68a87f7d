// Drop-in adapter: ORB_SLAM3::MLPnPsolver (reference include/MLPnPsolver.h, src/MLPnPsolver.cpp) over morb_mlpnp_solver_batch on the
// Optimizer's kTracking handle.  The reference's constructor is a member template on its Frame / MapPoint types (as in
// Optimizer_reference.h), so this header includes none of them; iterate writes the pose into any matrix with operator()(r, c)
// (Eigen::Matrix4f).
//   * Samples are drawn with rand() in the reference's order, minSet (six) per iteration, once per iterate call for that call's
//     iterations (mlpnp_call_end: to the end of the budget or nIterations more, whichever comes later; none when N < minInliers).
//     The one divergence: the reference stops drawing at the iteration whose Refine() succeeds, this adapter has drawn the whole
//     call's values by then.  rand() is process-global, so its position is not deterministic in the reference either.
//   * A minSet outside [6, 16] throws what the C ABI's argument error throws elsewhere (Optimizer::check).
#pragma once
#include <cstdlib>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "Optimizer.h"
#include "mlpnp_solver_math.h"
#include "ransac_math.h"

namespace ORB_SLAM3 {

class MLPnPsolver {
 public:
  // MLPnPsolver(const Frame& F, const vector<MapPoint*>& vpMapPointMatches)  MLPnPsolver.cpp:55-97
  template <class FrameT, class MP>
  MLPnPsolver(const FrameT& F, const std::vector<MP*>& vpMapPointMatches, int device = 0) : device_(device) {
    const int n = (int)vpMapPointMatches.size();
    n_ = n;
    entry_.assign(n, 0);
    uv_.assign((size_t)n * 2, 0.f);
    sigma2_.assign(n, 0.f);
    Xw_.assign((size_t)n * 3, 0.f);
    for (int i = 0; i < n; ++i) {
      MP* pMP = vpMapPointMatches[i];
      if (!pMP) continue;
      uint8_t e = 1;
      if (pMP->isBad()) e |= 2;
      if ((size_t)i >= F.mvKeysUn.size()) e |= 4;
      entry_[i] = e;
      if (e != 1) continue;   // the constructor reads nothing more of this match
      const auto& kp = F.mvKeysUn[i];
      uv_[(size_t)i * 2] = kp.pt.x; uv_[(size_t)i * 2 + 1] = kp.pt.y;
      sigma2_[i] = F.mvLevelSigma2[kp.octave];
      const auto X = pMP->GetWorldPos();
      for (int k = 0; k < 3; ++k) Xw_[(size_t)i * 3 + k] = X(k);
      ++N_;
    }
    morb_glue::cam8(F.mpCamera, params_.cam + 1);
    params_.cam[0] = F.mpCamera->size() >= 8 ? 1.f : 0.f;
    params_.n = n;
    SetRansacParameters();   // :96
  }

  // SetRansacParameters (:225-260).  Unlike Sim3Solver's it does not reset mnIterations, and neither does this.
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 6, float epsilon = 0.4,
                           float th2 = 5.991) {
    if (minSet < 6 || minSet > 16) throw std::runtime_error("MLPnPsolver::SetRansacParameters: minSet outside [6, 16]");
    params_.probability = probability;
    params_.minInliers = minInliers;
    params_.maxIterations = maxIterations;
    params_.minSet = minSet;
    params_.epsilon = epsilon;
    params_.th2 = th2;
    minInliers_ = morbpnp::mlpnp_min_inliers(N_, minInliers, minSet, epsilon);
    budget_ = morbransac::ransac_budget(N_, minInliers_, morbpnp::mlpnp_epsilon(N_, minInliers_, epsilon), probability, maxIterations);
  }

  // bool iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers, Eigen::Matrix4f& Tout)  (:100-223)
  template <class Mat4>
  bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, Mat4& Tout) {
    const int n = n_, minSet = params_.minSet;
    // the rand() values this call's iterations draw, in the reference's order
    const int it0 = state_.iterations;
    const int end = N_ >= minInliers_ ? morbpnp::mlpnp_call_end(it0, budget_, nIterations) : it0;
    if (rand_.size() < (size_t)end * minSet) rand_.resize((size_t)end * minSet, 0);
    for (size_t k = (size_t)it0 * minSet; k < (size_t)end * minSet; ++k) rand_[k] = std::rand();
    std::vector<uint8_t> mask(n > 0 ? n : 1, 0);
    if (n > 0) {
      if (best_.size() != (size_t)n) best_.assign(n, 0);
      Optimizer::Slot& o = Optimizer::slot(device_, Optimizer::kTracking);
      std::lock_guard<std::mutex> lock(o.mu);
      Optimizer::Call c(device_, morb_optimizer_stream(o.h));
      const int randCap = (int)rand_.size();
      const morb_mlpnp_solver_params* d_params = c.in(&params_, 1);
      const uint8_t* d_entry = c.in(entry_.data(), n);
      const float *d_uv = c.in(uv_.data(), (size_t)n * 2), *d_sigma2 = c.in(sigma2_.data(), n), *d_Xw = c.in(Xw_.data(), (size_t)n * 3);
      const int* d_rand = randCap > 0 ? c.in(rand_.data(), rand_.size()) : nullptr;
      morb_mlpnp_solver_state* d_state = c.in(&state_, 1);
      uint8_t* d_best = c.in(best_.data(), n);
      uint8_t* d_inliers = c.out<uint8_t>(n);
      Optimizer::check(morb_mlpnp_solver_batch(o.h, 1, n, d_params, d_entry, d_uv, d_sigma2, d_Xw, nIterations, d_rand, randCap, d_state, d_best,
                                               d_inliers, nullptr, 0, nullptr));
      c.wait();
      c.fetch(d_state, &state_, 1);
      c.fetch(d_best, best_.data(), n);
      c.fetch(d_inliers, mask.data(), n);
    } else {   // no match at all: N = 0 < minInliers
      state_.N = 0; state_.minInliers = minInliers_; state_.budget = budget_;
      state_.ok = 0; state_.noMore = 1; state_.nInliers = 0; state_.refined = 0; state_.returnedAt = -1;
      for (int i = 0; i < 16; ++i) state_.Tcw[i] = (i % 5 == 0) ? 1.f : 0.f;
    }
    bNoMore = state_.noMore != 0;
    nInliers = state_.nInliers;
    vbInliers.clear();   // the reference clears it and sizes it only on success
    if (state_.ok) {
      vbInliers.assign(n, false);
      for (int i = 0; i < n; ++i) vbInliers[i] = mask[i] != 0;
    }
    for (int r = 0; r < 4; ++r)
      for (int cc = 0; cc < 4; ++cc) Tout(r, cc) = state_.Tcw[r * 4 + cc];
    return state_.ok != 0;
  }

  const morb_mlpnp_solver_state& state() const { return state_; }

 private:
  int device_ = 0;
  int n_ = 0, N_ = 0, minInliers_ = 0, budget_ = 1;
  std::vector<uint8_t> entry_, best_;
  std::vector<float> uv_, sigma2_, Xw_;
  std::vector<int> rand_;
  morb_mlpnp_solver_params params_{};
  morb_mlpnp_solver_state state_{};
};

}  // namespace ORB_SLAM3
