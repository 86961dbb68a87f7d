// Scalar pieces of MLPnPsolver (reference src/MLPnPsolver.cpp) shared by the kernel (mlpnp_solver.hip), the C++ adapter
// (include/morb/MLPnPsolver.h) and the CPU tests: plain C++ that compiles for the host and for the device.
//   * mlpnp_min_inliers / mlpnp_epsilon / mlpnp_budget: SetRansacParameters (:225-260) from the constructor's N;
//   * mlpnp_max_error: sigma2 * th2 in float (:257-259);
//   * mlpnp_random_int: DUtils::Random::RandomInt(0, d - 1) on a rand() value;
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

// x86-64's cvttsd2si: a NaN or a value beyond int converts to INT_MIN, which the max(1, ..) clamp turns into a budget of 1
MORB_MLPNP_FN int cvt_i32_x86(double v) {
  if (!(v >= -2147483648.0 && v < 2147483648.0)) return (int)0x80000000u;
  return (int)v;
}

// mRansacMaxIts (:248-255): 1 when minInliers == N, else ceil(log(1 - p) / log(1 - pow(eps, 3))) (the exponent is 3, the minimal
// set 6), clipped to [1, maxIterations].  pow(float, int) is the double pow.
MORB_MLPNP_FN int mlpnp_budget(int N, int adjustedMinInliers, float adjustedEpsilon, double probability, int maxIterations) {
  int nIterations;
  if (adjustedMinInliers == N) nIterations = 1;
  else nIterations = cvt_i32_x86(ceil(log(1 - probability) / log(1 - pow((double)adjustedEpsilon, 3.0))));
  const int m = nIterations < maxIterations ? nIterations : maxIterations;
  return m > 1 ? m : 1;
}

MORB_MLPNP_FN float mlpnp_max_error(float sigma2, float th2) { return sigma2 * th2; }

// int(((double)r / ((double)RAND_MAX + 1.0)) * d) with RAND_MAX = 2^31 - 1: r * 2^-31 and r * d < 2^53 are exact, so (r * d) >> 31
MORB_MLPNP_FN int mlpnp_random_int(int r, int d) { return (int)(((uint64_t)(uint32_t)r * (uint64_t)(uint32_t)d) >> 31); }

// while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations): an OR, so a call runs to the end of the budget or
// nIterations iterations, whichever comes LATER; a call after the budget is spent still runs nIterations more.
MORB_MLPNP_FN int mlpnp_call_end(int iterationsDone, int budget, int nIterations) {
  const int byCount = iterationsDone + (nIterations > 0 ? nIterations : 0);
  const int end = budget > byCount ? budget : byCount;
  return end > iterationsDone ? end : iterationsDone;
}

}  // namespace morbpnp
