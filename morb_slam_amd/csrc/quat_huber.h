// The three device functions the SE3 optimisers (optimizer_device.h) and OptimizeSim3 (sim3.hip) both need, restated from Eigen and g2o;
// the projection searches (projection.hip) rotate with the first, in float.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// QuaternionBase::_transformVector; q = x y z w
template <class T>
__device__ __forceinline__ void q_rotate(const T* q, const T* v, T* out) {
  const T ux = q[0], uy = q[1], uz = q[2], w = q[3];
  T a = uy * v[2] - uz * v[1], b = uz * v[0] - ux * v[2], c = ux * v[1] - uy * v[0];
  a += a; b += b; c += c;
  out[0] = v[0] + w * a + (uy * c - uz * b);
  out[1] = v[1] + w * b + (uz * a - ux * c);
  out[2] = v[2] + w * c + (ux * b - uy * a);
}
// x^3 rounded once (up to a double rounding in rare cases): glibc's pow — what g2o's `pow(theta, 3)` and `pow(2 * rho - 1, 3)` call on the CPU — is
// accurate to ~0.52 ulp, x * x * x carries two roundings.  Error-free products through FMA, then one sum.
__device__ __forceinline__ double cube_rn(double x) {
  const double p = x * x, e = __builtin_fma(x, x, -p);      // x^2 = p + e
  const double q = p * x, f = __builtin_fma(p, x, -q);      // p x = q + f
  return q + (f + e * x);
}
// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): returns rho[0], *w = rho[1]
__device__ __forceinline__ double huber(double delta, double e, double* w) {
  const double dsqr = delta * delta;
  if (e <= dsqr) { *w = 1.0; return e; }
  const double sqrte = sqrt(e);
  *w = delta / sqrte;
  return 2 * sqrte * delta - dsqr;
}

}  // namespace
