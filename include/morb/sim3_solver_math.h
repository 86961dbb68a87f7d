// Scalar pieces of Sim3Solver (reference src/Sim3Solver.cc) shared by the kernel (sim3_solver.hip), the C++ adapter
// (include/morb/Sim3Solver.h) and the CPU tests: plain C++ that compiles for the host and for the device.
//   * sim3s_budget: SetRansacParameters (:122-146), mRansacMaxIts from N (the formula itself is ransac_math.h's);
//   * sim3s_max_error: 9.210 * sigma2 stored in a std::vector<size_t> (Sim3Solver.h:84-85, :98-99), i.e. truncated;
//   * sim3s_atan2: the double atan2 of ComputeSim3 (:335), fdlibm's e_atan2.c / s_atan.c.  The reference rounds 2 * atan2(..)
//     to float at once, so this restatement is held to that precision: tests/test_sim3_solver_cpu.py compares
//     (float)(2 * sim3s_atan2(y, x)) with the host libm's over float-valued arguments.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "ransac_math.h"

#if defined(__HIPCC__)
#define MORB_SIM3S_FN __host__ __device__ __forceinline__
#else
#define MORB_SIM3S_FN inline
#endif

namespace morbs3 {

// SetRansacParameters: epsilon = (float)minInliers / N, then the shared budget (N < minInliers gives a NaN ratio, minInliers / N
// below ~1.29e-3 one beyond 2^31: both a budget of 1)
MORB_SIM3S_FN int sim3s_budget(int N, int minInliers, double probability, int maxIterations) {
  const float epsilon = (float)minInliers / N;
  return morbransac::ransac_budget(N, minInliers, (double)epsilon, probability, maxIterations);
}

MORB_SIM3S_FN float sim3s_max_error(float sigma2) {   // (float)(size_t)(9.210 * sigma2)
  return (float)(uint64_t)(9.210 * (double)sigma2);
}

MORB_SIM3S_FN uint64_t d2u(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }

MORB_SIM3S_FN double atan_fdlibm(double x) {
  const double atanhi[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00};
  const double atanlo[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17};
  const double aT[11] = {3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
                         9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
                         4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02};
  const int32_t hx = (int32_t)(d2u(x) >> 32), ix = hx & 0x7fffffff;
  int id;
  if (ix >= 0x44100000) {   // |x| >= 2^66
    if (ix > 0x7ff00000 || (ix == 0x7ff00000 && (uint32_t)d2u(x) != 0)) return x + x;
    return hx > 0 ? atanhi[3] + atanlo[3] : -atanhi[3] - atanlo[3];
  }
  if (ix < 0x3fdc0000) {   // |x| < 0.4375
    if (ix < 0x3e200000) return x;   // |x| < 2^-29
    id = -1;
  } else {
    x = fabs(x);
    if (ix < 0x3ff30000) {
      if (ix < 0x3fe60000) { id = 0; x = (2.0 * x - 1.0) / (2.0 + x); }
      else { id = 1; x = (x - 1.0) / (x + 1.0); }
    } else {
      if (ix < 0x40038000) { id = 2; x = (x - 1.5) / (1.0 + 1.5 * x); }
      else { id = 3; x = -1.0 / x; }
    }
  }
  const double z = x * x, w = z * z;
  const double s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))));
  const double s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))));
  if (id < 0) return x - x * (s1 + s2);
  double r = 0;
  switch (id) {   // constant indices: no private array is addressed with a run-time index
    case 0: r = atanhi[0] - ((x * (s1 + s2) - atanlo[0]) - x); break;
    case 1: r = atanhi[1] - ((x * (s1 + s2) - atanlo[1]) - x); break;
    case 2: r = atanhi[2] - ((x * (s1 + s2) - atanlo[2]) - x); break;
    default: r = atanhi[3] - ((x * (s1 + s2) - atanlo[3]) - x); break;
  }
  return hx < 0 ? -r : r;
}

MORB_SIM3S_FN double sim3s_atan2(double y, double x) {
  const double tiny = 1.0e-300, pi_o_4 = 7.8539816339744827900E-01, pi_o_2 = 1.5707963267948965580E+00,
               pi = 3.1415926535897931160E+00, pi_lo = 1.2246467991473531772E-16;
  const uint64_t ux = d2u(x), uy = d2u(y);
  const int32_t hx = (int32_t)(ux >> 32), hy = (int32_t)(uy >> 32);
  const uint32_t lx = (uint32_t)ux, ly = (uint32_t)uy;
  const int32_t ix = hx & 0x7fffffff, iy = hy & 0x7fffffff;
  if (((uint32_t)ix | ((lx | (0u - lx)) >> 31)) > 0x7ff00000u || ((uint32_t)iy | ((ly | (0u - ly)) >> 31)) > 0x7ff00000u) return x + y;
  if ((((uint32_t)hx - 0x3ff00000u) | lx) == 0) return atan_fdlibm(y);   // x = 1
  const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);
  if ((iy | (int32_t)ly) == 0) {
    if (m <= 1) return y;
    return m == 2 ? pi + tiny : -pi - tiny;
  }
  if ((ix | (int32_t)lx) == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
  if (ix == 0x7ff00000) {
    if (iy == 0x7ff00000) {
      switch (m) {
        case 0: return pi_o_4 + tiny;
        case 1: return -pi_o_4 - tiny;
        case 2: return 3.0 * pi_o_4 + tiny;
        default: return -3.0 * pi_o_4 - tiny;
      }
    }
    switch (m) {
      case 0: return 0.0;
      case 1: return -0.0;
      case 2: return pi + tiny;
      default: return -pi - tiny;
    }
  }
  if (iy == 0x7ff00000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
  const int k = (iy - ix) >> 20;
  double z;
  if (k > 60) z = pi_o_2 + 0.5 * pi_lo;
  else if (hx < 0 && k < -60) z = 0.0;
  else z = atan_fdlibm(fabs(y / x));
  switch (m) {
    case 0: return z;
    case 1: return -z;
    case 2: return pi - (z - pi_lo);
    default: return (z - pi_lo) - pi;
  }
}

}  // namespace morbs3
