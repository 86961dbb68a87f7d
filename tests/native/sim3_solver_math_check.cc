// Host build of include/morb/sim3_solver_math.h (the scalar pieces the Sim3Solver kernel shares with the adapter) and of the
// RandomInt of ransac_math.h for tests/test_sim3_solver_cpu.py: the budget, the truncated thresholds, RandomInt and the double atan2
// restatement against the host libm.
#include <cmath>

#include "morb/sim3_solver_math.h"

extern "C" {
int ssm_budget(int N, int minInliers, double probability, int maxIterations) {
  return morbs3::sim3s_budget(N, minInliers, probability, maxIterations);
}
// log(1 - p) / log(1 - pow(eps, 3)) before ceil: the quantity whose last bits the device's log / pow may move
double ssm_budget_ratio(int N, int minInliers, double probability) {
  const float epsilon = (float)minInliers / N;
  return log(1 - probability) / log(1 - pow((double)epsilon, 3.0));
}
float ssm_max_error(float sigma2) { return morbs3::sim3s_max_error(sigma2); }
int ssm_random_int(int r, int d) { return morbransac::random_int(r, d); }
double ssm_atan2(double y, double x) { return morbs3::sim3s_atan2(y, x); }
// over n float pairs: how many differ from the host libm after the reference's use, (float)(2 * atan2(y, x)); and in all 64 bits
void ssm_atan2_check(int n, const float* y, const float* x, int* mismatchFloat, int* mismatchDouble) {
  int a = 0, b = 0;
  for (int i = 0; i < n; ++i) {
    const double r = morbs3::sim3s_atan2((double)y[i], (double)x[i]), h = atan2((double)y[i], (double)x[i]);
    const float fr = (float)(2 * r), fh = (float)(2 * h);
    if (!(fr == fh || (std::isnan(fr) && std::isnan(fh)))) a++;
    if (!(r == h || (std::isnan(r) && std::isnan(h)))) b++;
  }
  *mismatchFloat = a;
  *mismatchDouble = b;
}
}
