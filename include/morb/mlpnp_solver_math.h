// Scalar pieces of MLPnPsolver (reference src/MLPnPsolver.cpp) shared by the kernel (mlpnp_solver.hip), the C++ adapter
// (include/morb/MLPnPsolver.h) and the CPU tests: plain C++ that compiles for the host and for the device.
//   * mlpnp_min_inliers / mlpnp_epsilon: SetRansacParameters (:225-260) from the constructor's N; the budget (:248-255) is
//     morbransac::ransac_budget(N, mlpnp_min_inliers(..), mlpnp_epsilon(..), probability, maxIterations) of ransac_math.h;
//   * mlpnp_max_error: sigma2 * th2 in float (:257-259);
//   * mlpnp_call_end: the last iteration (exclusive) of one iterate(nIterations, ..) call, from its loop condition (:115).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MORB_MLPNP_FN __host__ __device__ __forceinline__
#else
#define MORB_MLPNP_FN inline
#endif

namespace morbpnp {

// int nMinInliers = N * mRansacEpsilon (a float product, truncated), raised to minInliers and to minSet (:237-242)
MORB_MLPNP_FN int mlpnp_min_inliers(int N, int minInliers, int minSet, float epsilon) {
  int m = (int)((float)N * epsilon);
  if (m < minInliers) m = minInliers;
  if (m < minSet) m = minSet;
  return m;
}

// mRansacEpsilon raised to (float)mRansacMinInliers / N (:244-245); N = 0 gives +inf, as in the reference
MORB_MLPNP_FN float mlpnp_epsilon(int N, int adjustedMinInliers, float epsilon) {
  const float e = (float)adjustedMinInliers / N;
  return epsilon < e ? e : epsilon;
}

MORB_MLPNP_FN float mlpnp_max_error(float sigma2, float th2) { return sigma2 * th2; }

// while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations): an OR, so a call runs to the end of the budget or
// nIterations iterations, whichever comes LATER; a call after the budget is spent still runs nIterations more.
MORB_MLPNP_FN int mlpnp_call_end(int iterationsDone, int budget, int nIterations) {
  const int byCount = iterationsDone + (nIterations > 0 ? nIterations : 0);
  const int end = budget > byCount ? budget : byCount;
  return end > iterationsDone ? end : iterationsDone;
}

}  // namespace morbpnp
