// g2o's Levenberg-Marquardt control flow with ORB-SLAM's stop rule (optimization_algorithm_levenberg.cpp:61-169 of the reference's g2o), as
// one record and two steps: lm_trial after every trial's chi2, lm_iteration_done after a trial loop has ended.  The arithmetic is the
// reference's, decision for decision; pow(2 rho - 1, 3) is cube_rn (quat_huber.h).  k_pose_opt, LocalBundleAdjustment, LocalInertialBA and
// OptimizeSim3 restated this loop inline before this header existed and keep their own text.  Behind the record: what the one-workgroup
// decision kernels of the four whole-map graph optimisers share — their state words, the two ordered sums and lane 0's decision.
#pragma once
#include <hip/hip_runtime.h>

#include "quat_huber.h"

namespace {

struct LmControl {
  double currentChi, iniChi, lambda, ni, rho;
  int qmax, nBad;
};

// first iteration: computeLambdaInit (user value when positive, else tau * max diagonal with tau = 1e-5)
__device__ __forceinline__ void lm_begin(LmControl& c, double userLambda, double maxDiagonal) {
  c.lambda = userLambda > 0 ? userLambda : 1e-5 * maxDiagonal;
  c.ni = 2;
  c.nBad = 0;
}
// start of an outer iteration, behind computeActiveErrors
__device__ __forceinline__ void lm_iteration(LmControl& c, double chi) { c.currentChi = chi; c.iniChi = chi; c.rho = 0; c.qmax = 0; }
// after one trial: tempChi = the trial state's chi2, ok2 = the factorisation succeeded, gain = computeScale() (sum x (lambda x + b)).
// Returns true when the step is kept; *again when another trial follows.  A NaN rho (NaN errors) is a rejected step that ends the loop.
__device__ __forceinline__ bool lm_trial(LmControl& c, double tempChi, bool ok2, double gain, bool* again) {
  if (!ok2) tempChi = 1.7976931348623157e308;
  c.rho = (c.currentChi - tempChi) / (gain + 1e-3);
  const bool keep = c.rho > 0 && isfinite(tempChi);
  if (keep) {
    double alpha = 1. - cube_rn(2 * c.rho - 1);
    alpha = fmin(alpha, 2. / 3.);
    c.lambda *= fmax(1. / 3., alpha);
    c.ni = 2;
    c.currentChi = tempChi;
  } else {
    c.lambda *= c.ni;
    c.ni *= 2;
  }
  ++c.qmax;
  *again = c.rho < 0 && c.qmax < 10;
  return keep;
}
// after the trial loop: true when the optimisation ends (ten trials, rho == 0 or NaN, or three stagnant iterations in a row)
__device__ __forceinline__ bool lm_iteration_done(LmControl& c) {
  if (c.qmax == 10 || c.rho == 0 || !(c.rho == c.rho)) return true;
  if ((c.iniChi - c.currentChi) * 1e3 < c.iniChi) c.nBad++; else c.nBad = 0;
  return c.nBad >= 3;
}

// ---- the decision kernel of the four whole-map graph optimisers (essential graph, 4-DoF pose graph, global BA, full inertial BA) ----
// their `lmi` words on the device; LMW_LAMBDA0 only where the first lambda waits for the first assembly's max diagonal
enum { LMW_DONE = 0, LMW_REBUILD, LMW_ITS, LMW_TRIALS, LMW_OK2, LMW_LAMBDA0 };

// Sum of n values strictly in index order: the workgroup of NT stages SUM of them in LDS (buf[SUM]) at a time, lane 0 adds.  term(i) is
// evaluated by every lane; the result is lane 0's.
template <int NT, int SUM, class Term>
__device__ double lm_sum_in_index_order(double* buf, int n, Term&& term) {
  double acc = 0;
  for (int base = 0; base < n; base += SUM) {
    const int m = min(SUM, n - base);
    for (int q = threadIdx.x; q < m; q += NT) buf[q] = term(base + q);
    __syncthreads();
    if (threadIdx.x == 0)
      for (int q = 0; q < m; ++q) acc += buf[q];
    __syncthreads();
  }
  return acc;
}
// Sum of n values by lane slices: lane t adds its slice of ceil(n / NT) consecutive values, lane 0 adds the lanes' sums (buf[NT]) in lane
// order.  A fixed order, but not the index order's rounding.  The result is lane 0's.
template <int NT, class Term>
__device__ double lm_sum_of_lane_slices(double* buf, int n, Term&& term) {
  const int per = (n + NT - 1) / NT, t = threadIdx.x;
  double s = 0;
  for (int i = t * per; i < min((t + 1) * per, n); ++i) s += term(i);
  __syncthreads();
  buf[t] = s;
  __syncthreads();
  double acc = 0;
  if (t == 0)
    for (int q = 0; q < NT; ++q) acc += buf[q];
  return acc;
}

// Lane 0 behind a trial: g2o's decision on the trial's chi2, the iteration count and the end of the optimisation (stop: the caller's
// stop flag as read now; an optimiser without one passes false), written to *lm, chi2[1] and the lmi words, then mirrored to the mapped
// host words lmHost ([1] done, [0] decided trials).  Returns true when the trial state is kept.
__device__ __forceinline__ bool lm_decide_trial(LmControl c, double chi, bool ok2, double gain, bool stop, int maxIts, LmControl* lm,
                                                double* chi2, int* lmi, int* lmHost) {
  bool again = false;
  const bool keep = lm_trial(c, chi, ok2, gain, &again);
  if (stop) again = false;
  int its = lmi[LMW_ITS], done = 0, rebuild = 0;
  const int trials = lmi[LMW_TRIALS] + 1;
  if (!again) {
    ++its;
    done = (lm_iteration_done(c) || its >= maxIts || stop) ? 1 : 0;
    if (!done) { lm_iteration(c, c.currentChi); rebuild = 1; }
  }
  *lm = c;
  chi2[1] = c.currentChi;
  lmi[LMW_ITS] = its; lmi[LMW_TRIALS] = trials; lmi[LMW_REBUILD] = rebuild; lmi[LMW_DONE] = done;
  __hip_atomic_store(lmHost + 1, done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(lmHost + 0, trials, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // decided trials: the host queues trial k + 2 when it sees k
  return keep;
}

}  // namespace
