// g2o's Levenberg-Marquardt control flow with ORB-SLAM's stop rule (optimization_algorithm_levenberg.cpp:61-169 of the reference's g2o), as
// one record and two steps: lm_trial after every trial's chi2, lm_iteration_done after a trial loop has ended.  The arithmetic is the
// reference's, decision for decision; pow(2 rho - 1, 3) is cube_rn (quat_huber.h).  k_pose_opt, LocalBundleAdjustment, LocalInertialBA and
// OptimizeSim3 restated this loop inline before this header existed and keep their own text.
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

}  // namespace
