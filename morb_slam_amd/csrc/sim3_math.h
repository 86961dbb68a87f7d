// The Sim3 algebra of g2o (types/sim3.h) and the Eigen pieces under it, restated operation for operation in FP64 for the two units that
// optimise over Sim3: OptimizeSim3 (sim3.hip) and OptimizeEssentialGraph (essential_graph.hip).  sin / cos / exp are glibc's (libm_f64.h).
#pragma once
#include <hip/hip_runtime.h>

#include "libm_f64.h"
#include "quat_huber.h"

namespace {

constexpr double S3_DELTA = 1e-9;   // the step of g2o's numeric Jacobians (base_binary_edge.hpp, base_unary_edge.hpp)

struct Sim3d { double q[4]; double t[3]; double s; };   // q = x y z w

// ---- Eigen / g2o Sim3 algebra ------------------------------------------------------------------------------
__device__ __forceinline__ void q_mul(const double* p, const double* o, double* r) {   // quat_product (generic)
  r[3] = p[3] * o[3] - p[0] * o[0] - p[1] * o[1] - p[2] * o[2];
  r[0] = p[3] * o[0] + p[0] * o[3] + p[1] * o[2] - p[2] * o[1];
  r[1] = p[3] * o[1] + p[1] * o[3] + p[2] * o[0] - p[0] * o[2];
  r[2] = p[3] * o[2] + p[2] * o[3] + p[0] * o[1] - p[1] * o[0];
}
// Quaterniond(Matrix3d) (Eigen Quaternion.h, quaternionbase_assign_impl)
__device__ __forceinline__ void R_to_q(const double* m, double* q) {
  double t = m[0] + m[4] + m[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t;
    q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
    q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
  }
}
__device__ __forceinline__ Sim3d sim3_mul(const Sim3d& a, const Sim3d& b) {   // Sim3::operator*
  Sim3d r;
  q_mul(a.q, b.q, r.q);
  double rt[3];
  q_rotate(a.q, b.t, rt);
  for (int i = 0; i < 3; ++i) r.t[i] = a.s * rt[i] + a.t[i];
  r.s = a.s * b.s;
  return r;
}
__device__ __forceinline__ void sim3_map(const Sim3d& S, const double* x, double* o) {   // s * (r * x) + t
  double r[3];
  q_rotate(S.q, x, r);
  for (int i = 0; i < 3; ++i) o[i] = S.s * r[i] + S.t[i];
}
__device__ __forceinline__ Sim3d sim3_inverse(const Sim3d& S) {   // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
  Sim3d r;
  r.q[0] = -S.q[0]; r.q[1] = -S.q[1]; r.q[2] = -S.q[2]; r.q[3] = S.q[3];
  const double ms = -1. / S.s;
  const double v[3] = {ms * S.t[0], ms * S.t[1], ms * S.t[2]};
  q_rotate(r.q, v, r.t);
  r.s = 1. / S.s;
  return r;
}
// Sim3(const Vector7d& update) (types/sim3.h); s = exp(update[6]) is passed in
__device__ Sim3d sim3_exp(const double* u, double s) {
  const double w0 = u[0], w1 = u[1], w2 = u[2], sigma = u[6];
  const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
  const double Om[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
  double Om2[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Om2[i * 3 + j] = Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j] + Om[i * 3 + 2] * Om[6 + j];
  const double eps = 0.00001;
  double A, B, C, R[9];
  bool smallRot = theta < eps;
  if (fabs(sigma) < eps) {
    C = 1;
    if (smallRot) { A = 1. / 2.; B = 1. / 6.; }
    else {
      const double sn = morbm64::sin_glibc(theta), cs = morbm64::cos_glibc(theta);
      const double theta2 = theta * theta;
      A = (1 - cs) / (theta2);
      B = (theta - sn) / (theta2 * theta);
    }
  } else {
    C = (s - 1) / sigma;
    if (smallRot) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
    } else {
      const double sn = morbm64::sin_glibc(theta), cs = morbm64::cos_glibc(theta);
      const double a = s * sn, b = s * cs;
      const double theta2 = theta * theta, sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  if (smallRot) {
    for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + Om[i] + Om2[i];
  } else {
    const double sn = morbm64::sin_glibc(theta), cs = morbm64::cos_glibc(theta);
    const double f1 = sn / theta, f2 = (1 - cs) / (theta * theta);
    for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + f1 * Om[i] + f2 * Om2[i];
  }
  Sim3d r;
  R_to_q(R, r.q);
  double W[9];
  for (int i = 0; i < 9; ++i) W[i] = A * Om[i] + B * Om2[i] + C * ((i % 4 == 0) ? 1.0 : 0.0);
  for (int i = 0; i < 3; ++i) r.t[i] = W[i * 3] * u[3] + W[i * 3 + 1] * u[4] + W[i * 3 + 2] * u[5];
  r.s = s;
  return r;
}

}  // namespace
