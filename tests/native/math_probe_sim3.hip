// Test-only probe, the sim3_math.h family: Eigen's matrix -> quaternion in its run-time index form, g2o's Sim3 exponential with its
// four |sigma| < eps x smallRot branches, and the Sim3 product, inverse and map.  Part of tests/native/libmath_probe.so.
#include "math_probe_common.h"

#include "sim3_math.h"

// Sim3 records: q (x y z w), t, s
namespace {
__device__ __forceinline__ Sim3d ld_sim3(const double* a) { Sim3d S; for (int k = 0; k < 4; ++k) S.q[k] = a[k]; for (int k = 0; k < 3; ++k) S.t[k] = a[4 + k]; S.s = a[7]; return S; }
__device__ __forceinline__ void st_sim3(const Sim3d& S, double* o) { for (int k = 0; k < 4; ++k) o[k] = S.q[k]; for (int k = 0; k < 3; ++k) o[4 + k] = S.t[k]; o[7] = S.s; }
}  // namespace

PROBE(R_to_q_sim3, double, 9, double, 4, R_to_q(a, o);)
// the 7-vector update (omega, upsilon, sigma); s = exp(sigma) as the callers compute it (libm_f64.h), returned in the record
PROBE(sim3_exp, double, 7, double, 8, st_sim3(sim3_exp(a, morbm64::exp_glibc(a[6])), o);)
PROBE(sim3_mul, double, 16, double, 8, st_sim3(sim3_mul(ld_sim3(a), ld_sim3(a + 8)), o);)
PROBE(sim3_inverse, double, 8, double, 8, st_sim3(sim3_inverse(ld_sim3(a)), o);)
PROBE(sim3_map, double, 11, double, 3, sim3_map(ld_sim3(a), a + 8, o);)
// S * S^-1 applied to a point: the point again
PROBE(sim3_roundtrip, double, 11, double, 3, const Sim3d S = ld_sim3(a); sim3_map(sim3_mul(S, sim3_inverse(S)), a + 8, o);)
