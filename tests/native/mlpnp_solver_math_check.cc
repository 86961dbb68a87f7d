// The scalar pieces of include/morb/mlpnp_solver_math.h (and the budget of ransac_math.h, as the solver forms its arguments) behind
// a C interface, for tests/test_mlpnp_solver_cpu.py.
#include "morb/mlpnp_solver_math.h"
#include "morb/ransac_math.h"

extern "C" {
// out: adjusted minInliers, budget
void mpm_ransac(int N, int minInliers, int maxIterations, int minSet, float epsilon, double probability, int* out) {
  const int m = morbpnp::mlpnp_min_inliers(N, minInliers, minSet, epsilon);
  out[0] = m;
  out[1] = morbransac::ransac_budget(N, m, morbpnp::mlpnp_epsilon(N, m, epsilon), probability, maxIterations);
}
float mpm_max_error(float sigma2, float th2) { return morbpnp::mlpnp_max_error(sigma2, th2); }
int mpm_call_end(int done, int budget, int nIterations) { return morbpnp::mlpnp_call_end(done, budget, nIterations); }
}
