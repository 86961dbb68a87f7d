// Scalar pieces the three RANSAC solvers of the reference share (Sim3Solver, MLPnPsolver, TwoViewReconstruction), used by their
// kernels, their C++ adapters and the CPU tests: plain C++ that compiles for the host and for the device.
//   * random_int: DUtils::Random::RandomInt(0, d - 1) on a rand() value;
//   * cvt_i32_x86: the double -> int conversion as x86-64 performs it;
//   * ransac_budget: mRansacMaxIts of Sim3Solver::SetRansacParameters (:122-146) and MLPnPsolver::SetRansacParameters (:248-255).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MORB_RANSAC_FN __host__ __device__ __forceinline__
#else
#define MORB_RANSAC_FN inline
#endif

namespace morbransac {

// int(((double)r / ((double)RAND_MAX + 1.0)) * d): RAND_MAX = 2^31 - 1 (glibc), so the quotient is r * 2^-31 exactly and the
// product r * d < 2^53 is exact too: the index is (r * d) >> 31.
MORB_RANSAC_FN int random_int(int r, int d) { return (int)(((uint64_t)(uint32_t)r * (uint64_t)(uint32_t)d) >> 31); }

// x86-64's cvttsd2si: a NaN or a value beyond int converts to INT_MIN
MORB_RANSAC_FN int cvt_i32_x86(double v) {
  if (!(v >= -2147483648.0 && v < 2147483648.0)) return (int)0x80000000u;
  return (int)v;
}

// nIterations = minInliers == N ? 1 : ceil(log(1 - p) / log(1 - pow(epsilon, 3))), clipped to [1, maxIterations].  epsilon is the
// solver's float ratio and pow(float, int) the double pow; the exponent is 3 in both solvers (MLPnP's minimal set is 6).  A NaN
// ratio (N < minInliers, N = 0) or one beyond 2^31 (epsilon below ~1.29e-3) converts to INT_MIN, which the max(1, ..) clamp
// turns into a budget of 1.  Eps is float, or double where the caller has widened the float already (sim3s_budget): the value
// is the same, and where the widening stands (before or behind log(1 - p)) decides the instruction order of the kernel around
// it, which is pinned per kernel.
template <class Eps>
MORB_RANSAC_FN int ransac_budget(int N, int minInliers, Eps epsilon, double probability, int maxIterations) {
  int nIterations;
  if (minInliers == N) nIterations = 1;
  else nIterations = cvt_i32_x86(ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3.0))));
  const int m = nIterations < maxIterations ? nIterations : maxIterations;
  return m > 1 ? m : 1;
}

}  // namespace morbransac
