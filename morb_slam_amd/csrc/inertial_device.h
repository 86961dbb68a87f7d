// Device helpers the visual-inertial tracking slice (inertial.hip) and LocalInertialBA (inertial_ba.hip) share: the 3 x 3 helpers (FP32 for the
// preintegrated deltas, FP64 elsewhere), the SO(3) pieces, the small dense inverse and eigenvalue clamp, ImuCamPose (CamGeom, VIState) with its visual edge, and
// EdgeInertial (imu_delta, inertial_edge); make_geom fills CamGeom on the host.  What only one of the two uses lives in that unit.
// Everything is in an unnamed namespace: each unit gets its own copy, and the kernels keep their mangled names.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "libm_f32.h"
#include "morb/camera_math.h"
#include "morb_hip.h"
#include "wave.h"

namespace {

// ---- 3x3 helpers in FP32 (the reference preintegrates in float) and FP64 ---------------------------------------------------
template <class T>
__device__ __forceinline__ void mul33(const T* A, const T* B, T* C) {
  T P[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) P[r * 3 + c] = A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c] + A[r * 3 + 2] * B[6 + c];
#pragma unroll
  for (int k = 0; k < 9; ++k) C[k] = P[k];
}
template <class T>
__device__ __forceinline__ void mul3v(const T* A, const T* v, T* o) {
  T t[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) t[r] = A[r * 3] * v[0] + A[r * 3 + 1] * v[1] + A[r * 3 + 2] * v[2];
  o[0] = t[0]; o[1] = t[1]; o[2] = t[2];
}
__device__ __forceinline__ void hatf(const float* v, float* W) {
  W[0] = 0; W[1] = -v[2]; W[2] = v[1]; W[3] = v[2]; W[4] = 0; W[5] = -v[0]; W[6] = -v[1]; W[7] = v[0]; W[8] = 0;
}
// NormalizeRotation (ImuTypes.cc:35-39: U V^T of the SVD) = polar factor; Newton iteration X <- (X + X^-T) / 2 in FP64
__device__ void normalize_rotation_f(float* R) {
  double X[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) X[k] = R[k];
  for (int it = 0; it < 3; ++it) {   // quadratic convergence from a float-rounded rotation: 1e-7 -> 1e-14 -> below FP64 rounding
    const double c00 = X[4] * X[8] - X[5] * X[7], c01 = X[5] * X[6] - X[3] * X[8], c02 = X[3] * X[7] - X[4] * X[6];
    const double inv = 1.0 / (X[0] * c00 + X[1] * c01 + X[2] * c02);
    const double C[9] = {c00, c01, c02,
                         X[2] * X[7] - X[1] * X[8], X[0] * X[8] - X[2] * X[6], X[1] * X[6] - X[0] * X[7],
                         X[1] * X[5] - X[2] * X[4], X[2] * X[3] - X[0] * X[5], X[0] * X[4] - X[1] * X[3]};
#pragma unroll
    for (int k = 0; k < 9; ++k) X[k] = 0.5 * (X[k] + C[k] * inv);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = (float)X[k];
}

// ---- FP64 pieces ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void transpose33(const double* A, double* T) {
  double t[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) t[r * 3 + c] = A[c * 3 + r];
#pragma unroll
  for (int k = 0; k < 9; ++k) T[k] = t[k];
}
__device__ void exp_so3(const double* w, double* R) {   // ExpSO3, G2oTypes.cc:783-796
  const double x = w[0], y = w[1], z = w[2];
  const double d2 = x * x + y * y + z * z, d = sqrt(d2);
  const double W[9] = {0, -z, y, z, 0, -x, -y, x, 0};
  double WW[9];
  mul33(W, W, WW);
  if (d < 1e-5) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = ((k & 3) == 0 ? 1.0 : 0.0) + W[k] + 0.5 * WW[k];
  } else {
    const double s = sin(d), c = cos(d);
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = ((k & 3) == 0 ? 1.0 : 0.0) + W[k] * s / d + WW[k] * (1.0 - c) / d2;
  }
}
__device__ void log_so3(const double* R, double* w) {   // LogSO3, G2oTypes.cc:798-811
  const double tr = R[0] + R[4] + R[8];
  w[0] = (R[7] - R[5]) / 2; w[1] = (R[2] - R[6]) / 2; w[2] = (R[3] - R[1]) / 2;
  const double costheta = (tr - 1.0) * 0.5f;
  if (costheta > 1 || costheta < -1) return;
  const double theta = acos(costheta), s = sin(theta);
  if (fabs(s) < 1e-5) return;
  for (int k = 0; k < 3; ++k) w[k] = theta * w[k] / s;
}
__device__ void inv_right_jacobian_so3(const double* v, double* J) {   // G2oTypes.cc:817-829
  const double x = v[0], y = v[1], z = v[2];
  const double d2 = x * x + y * y + z * z, d = sqrt(d2);
  const double W[9] = {0, -z, y, z, 0, -x, -y, x, 0};
  if (d < 1e-5) { for (int k = 0; k < 9; ++k) J[k] = (k & 3) == 0 ? 1.0 : 0.0; return; }
  double WW[9];
  mul33(W, W, WW);
  const double k2 = 1.0 / d2 - (1.0 + cos(d)) / (2.0 * d * sin(d));
  for (int k = 0; k < 9; ++k) J[k] = ((k & 3) == 0 ? 1.0 : 0.0) + W[k] / 2 + WW[k] * k2;
}

__device__ __forceinline__ double wave_sum(double v) { return morbwave::sum_f64(v); }   // DPP, no LDS-crossbar round trips

__device__ void right_jacobian_so3(const double* v, double* J) {   // G2oTypes.cc:835-848
  const double x = v[0], y = v[1], z = v[2];
  const double d2 = x * x + y * y + z * z, d = sqrt(d2);
  const double W[9] = {0, -z, y, z, 0, -x, -y, x, 0};
  if (d < 1e-5) { for (int k = 0; k < 9; ++k) J[k] = (k & 3) == 0 ? 1.0 : 0.0; return; }
  double WW[9];
  mul33(W, W, WW);
  for (int k = 0; k < 9; ++k) J[k] = ((k & 3) == 0 ? 1.0 : 0.0) - W[k] * (1.0 - cos(d)) / d2 + WW[k] * (d - sin(d)) / (d2 * d);
}

// n x n inverse (Gauss-Jordan, partial pivoting); M is n x 2n scratch.  One thread.
__device__ bool invert_n(const double* A, int n, double* Ainv, double* M) {
  for (int r = 0; r < n; ++r) for (int c = 0; c < 2 * n; ++c) M[r * 2 * n + c] = c < n ? A[r * n + c] : (c - n == r ? 1.0 : 0.0);
  for (int c = 0; c < n; ++c) {
    int p = c;
    for (int r = c + 1; r < n; ++r) if (fabs(M[r * 2 * n + c]) > fabs(M[p * 2 * n + c])) p = r;
    if (M[p * 2 * n + c] == 0.0) return false;
    if (p != c) for (int k = 0; k < 2 * n; ++k) { const double t = M[p * 2 * n + k]; M[p * 2 * n + k] = M[c * 2 * n + k]; M[c * 2 * n + k] = t; }
    const double inv = 1.0 / M[c * 2 * n + c];
    for (int k = 0; k < 2 * n; ++k) M[c * 2 * n + k] *= inv;
    for (int r = 0; r < n; ++r) {
      if (r == c) continue;
      const double f = M[r * 2 * n + c];
      if (f != 0.0) for (int k = 0; k < 2 * n; ++k) M[r * 2 * n + k] -= f * M[c * 2 * n + k];
    }
  }
  for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) Ainv[r * n + c] = M[r * 2 * n + n + c];
  return true;
}
// S (n x n, symmetric) <- V max(e, clamp) V^T with eigenvalues below `thr` set to zero (EdgeInertial's information,
// G2oTypes.cc:484-491; ConstraintPoseImu, G2oTypes.h:715-720).  The rebuild only changes S when such an eigenvalue exists:
// S - thr I positive definite (LDL^T test) <=> none does; the cyclic-Jacobi rebuild runs otherwise.  One thread; A, V: n x n scratch.
__device__ void clamp_eigenvalues(double* S, int n, double thr, double* A, double* V) {
  bool pd = true;
  for (int k = 0; k < n * n; ++k) A[k] = S[k];
  for (int k = 0; k < n; ++k) A[k * n + k] -= thr;
  for (int j = 0; j < n && pd; ++j) {
    const double d = A[j * n + j];
    if (!(d > 0)) { pd = false; break; }
    for (int r = n - 1; r > j; --r) {       // descending rows: A[c][j] for c < r is still the un-scaled column entry
      const double l = A[r * n + j] / d;
      for (int c = j + 1; c <= r; ++c) A[r * n + c] -= l * A[c * n + j];
    }
  }
  if (pd) return;
  for (int k = 0; k < n * n; ++k) { A[k] = S[k]; V[k] = 0.0; }
  for (int k = 0; k < n; ++k) V[k * n + k] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0, diag = 0;
    for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) { const double t = A[r * n + c] * A[r * n + c]; if (r == c) diag += t; else off += t; }
    if (off <= 1e-30 * diag) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        if (A[p * n + q] == 0.0) continue;
        const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * A[p * n + q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) { const double a = A[k * n + p], bq = A[k * n + q]; A[k * n + p] = c * a - s * bq; A[k * n + q] = s * a + c * bq; }
        for (int k = 0; k < n; ++k) { const double a = A[p * n + k], bq = A[q * n + k]; A[p * n + k] = c * a - s * bq; A[q * n + k] = s * a + c * bq; }
        for (int k = 0; k < n; ++k) { const double a = V[k * n + p], bq = V[k * n + q]; V[k * n + p] = c * a - s * bq; V[k * n + q] = s * a + c * bq; }
      }
  }
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) {
      double s = 0;
      for (int k = 0; k < n; ++k) { const double e = A[k * n + k] < thr ? 0.0 : A[k * n + k]; s += V[r * n + k] * e * V[c * n + k]; }
      S[r * n + c] = s;
    }
}

// camera 0 = the pinhole camera, or on a fisheye rig (rig != 0) the left KannalaBrandt8 camera with camera 1 = the right one
// (ImuCamPose, G2oTypes.cc:74-118: Rcb[1] = Rrl Rcb[0], tcb[1] = Rrl tcb[0] + trl)
struct CamGeom {
  double Rcb[9], tcb[3], Rbc[9], tbc[3], bf;
  float fx, fy, cx, cy;
  int rig;
  float kb[2][8];
  double Rcb1[9], tcb1[3], Rbc1[9], tbc1[3];
};

struct VIState {
  double Rwb[9], twb[3], v[3], bg[3], ba[3];
  double Rcw[9], tcw[3];
  double Rcw1[9], tcw1[3];   // right camera of a rig
};
template <bool RIG>
__device__ __forceinline__ void refresh_camera_t(const CamGeom& g, VIState& S) {   // G2oTypes.cc:209-215
  double Rbw[9], tbw[3];
  transpose33(S.Rwb, Rbw);
  mul3v(Rbw, S.twb, tbw);
  for (int k = 0; k < 3; ++k) tbw[k] = -tbw[k];
  mul33(g.Rcb, Rbw, S.Rcw);
  mul3v(g.Rcb, tbw, S.tcw);
  for (int k = 0; k < 3; ++k) S.tcw[k] += g.tcb[k];
  if (RIG) {
    mul33(g.Rcb1, Rbw, S.Rcw1);
    mul3v(g.Rcb1, tbw, S.tcw1);
    for (int k = 0; k < 3; ++k) S.tcw1[k] += g.tcb1[k];
  }
}
// RIG as a template parameter keeps the right camera's pose out of the registers of the pinhole instantiations
__device__ __forceinline__ void refresh_camera(const CamGeom& g, VIState& S) { if (g.rig) refresh_camera_t<true>(g, S); else refresh_camera_t<false>(g, S); }
template <bool RIG>
__device__ __forceinline__ void load_state_t(const CamGeom& g, const float* s0, VIState& S) {
  for (int k = 0; k < 9; ++k) S.Rwb[k] = s0[k];
  for (int k = 0; k < 3; ++k) { S.twb[k] = s0[9 + k]; S.v[k] = s0[12 + k]; S.bg[k] = s0[15 + k]; S.ba[k] = s0[18 + k]; }
  refresh_camera_t<RIG>(g, S);
}
__device__ __forceinline__ void load_state(const CamGeom& g, const float* s0, VIState& S) { if (g.rig) load_state_t<true>(g, s0, S); else load_state_t<false>(g, s0, S); }
template <bool RIG>
__device__ __forceinline__ void apply_update_t(const CamGeom& g, VIState& S, const double* x) {   // ImuCamPose::Update + the additive vertices
  double t[3], dR[9];
  mul3v(S.Rwb, x + 3, t);
  for (int k = 0; k < 3; ++k) S.twb[k] += t[k];
  exp_so3(x, dR);
  mul33(S.Rwb, dR, S.Rwb);
  refresh_camera_t<RIG>(g, S);
  for (int k = 0; k < 3; ++k) { S.v[k] += x[6 + k]; S.bg[k] += x[9 + k]; S.ba[k] += x[12 + k]; }
}
__device__ __forceinline__ void apply_update(const CamGeom& g, VIState& S, const double* x) { if (g.rig) apply_update_t<true>(g, S, x); else apply_update_t<false>(g, S, x); }
// visual edge: error (obs - projection) and chi2; st = stereo
// the edge camera's KannalaBrandt8 parameters picked element by element: `g.kb[cam]` with a per-lane index made the compiler copy the whole
// CamGeom kernel argument to scratch memory to index it (736 B per thread in the rig kernels)
__device__ __forceinline__ void kb_of(const CamGeom& g, int cam, float (&p)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) p[i] = cam ? g.kb[1][i] : g.kb[0][i];
}
template <bool RIG>
__device__ __forceinline__ double vis_error_t(const CamGeom& g, const VIState& S, const double* X, const float* o, bool st, double info,
                                              double* err, double* Xc, int cam) {
  if (RIG && cam) { mul3v(S.Rcw1, X, Xc); for (int k = 0; k < 3; ++k) Xc[k] += S.tcw1[k]; }
  else { mul3v(S.Rcw, X, Xc); for (int k = 0; k < 3; ++k) Xc[k] += S.tcw[k]; }
  double u, v;
  if (RIG) { double uv[2]; float kp[8]; kb_of(g, cam, kp); morbcam::kb8_project_d(kp, Xc, uv); u = uv[0]; v = uv[1]; }   // KannalaBrandt8::project(Vector3d)
  else { u = g.fx * Xc[0] / Xc[2] + g.cx; v = g.fy * Xc[1] / Xc[2] + g.cy; }                       // Pinhole.cpp:38-44
  err[0] = (double)o[0] - u; err[1] = (double)o[1] - v; err[2] = 0;
  double c = err[0] * info * err[0] + err[1] * info * err[1];
  if (st) { const double invZ = 1 / Xc[2]; err[2] = (double)o[2] - (u - g.bf * invZ); c += err[2] * info * err[2]; }
  return c;
}
__device__ __forceinline__ double vis_error(const CamGeom& g, const VIState& S, const double* X, const float* o, bool st, double info,
                                            double* err, double* Xc, int cam = 0) {
  return g.rig ? vis_error_t<true>(g, S, X, o, st, info, err, Xc, cam) : vis_error_t<false>(g, S, X, o, st, info, err, Xc, 0);
}
// projectJac of the edge's camera (2 x 3 in pj[0..5]); pinhole: Pinhole.cpp:76-86
template <bool RIG>
__device__ __forceinline__ void cam_project_jac_t(const CamGeom& g, const double* Xc, int cam, double* pj) {
  if (RIG) { float kp[8]; kb_of(g, cam, kp); morbcam::kb8_project_jac(kp, Xc, pj); return; }
  pj[0] = g.fx / Xc[2]; pj[1] = 0; pj[2] = -g.fx * Xc[0] / (Xc[2] * Xc[2]);
  pj[3] = 0; pj[4] = g.fy / Xc[2]; pj[5] = -g.fy * Xc[1] / (Xc[2] * Xc[2]);
}
__device__ __forceinline__ void cam_project_jac(const CamGeom& g, const double* Xc, int cam, double* pj) {
  if (g.rig) cam_project_jac_t<true>(g, Xc, cam, pj); else cam_project_jac_t<false>(g, Xc, 0, pj);
}
template <bool RIG>
__device__ __forceinline__ void vis_jacobian_t(const CamGeom& g, const double* Xc, bool st, double* J /*[3][6]*/, int cam) {   // G2oTypes.cc:361-442
  double Xb[3];
  const bool c1 = RIG && cam;
  // (element-wise selects: a pointer chosen between two members of the kernel-argument struct sends the struct to scratch memory)
  double Rbc[9], tbc[3], Rcb[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) { Rbc[k] = c1 ? g.Rbc1[k] : g.Rbc[k]; Rcb[k] = c1 ? g.Rcb1[k] : g.Rcb[k]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) tbc[k] = c1 ? g.tbc1[k] : g.tbc[k];
  mul3v(Rbc, Xc, Xb);
  for (int k = 0; k < 3; ++k) Xb[k] += tbc[k];
  double pj[9];
  cam_project_jac_t<RIG>(g, Xc, cam, pj);
  pj[6] = pj[7] = pj[8] = 0;
  if (st) { pj[6] = pj[0]; pj[7] = pj[1]; pj[8] = pj[2] + g.bf * (1.0 / (Xc[2] * Xc[2])); }
  const double x = Xb[0], y = Xb[1], z = Xb[2];
  // J = (proj_jac Rcb) [ -[Xb]x | I ]: SE3deriv = {0, z, -y, 1, 0, 0; -z, 0, x, 0, 1, 0; y, -x, 0, 0, 0, 1} written out — its zeros and ones cost 63 of an
  // edge's ~300 FP64 instructions when multiplied through (x * 0.0 does not fold); the same values (a + 0 = a, a * 1 = a)
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double PR[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) PR[c] = pj[r * 3] * Rcb[c] + pj[r * 3 + 1] * Rcb[3 + c] + pj[r * 3 + 2] * Rcb[6 + c];
    J[r * 6 + 0] = PR[1] * -z + PR[2] * y;
    J[r * 6 + 1] = PR[0] * z + PR[2] * -x;
    J[r * 6 + 2] = PR[0] * -y + PR[1] * x;
    J[r * 6 + 3] = PR[0]; J[r * 6 + 4] = PR[1]; J[r * 6 + 5] = PR[2];
  }
}
__device__ __forceinline__ void vis_jacobian(const CamGeom& g, const double* Xc, bool st, double* J, int cam = 0) {
  if (g.rig) vis_jacobian_t<true>(g, Xc, st, J, cam); else vis_jacobian_t<false>(g, Xc, st, J, 0);
}
__device__ __forceinline__ double huber_w(double delta, double e2) {   // rho'(e2), robust_kernel_impl.cpp:65-91
  return e2 <= delta * delta ? 1.0 : delta / sqrt(e2);
}
__device__ __forceinline__ void put33(double* J, int ld, int r0, int c0, const double* B, double sgn) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) J[(r0 + r) * ld + c0 + c] = sgn * B[r * 3 + c];
}
// GetDeltaRotation / GetDeltaVelocity / GetDeltaPosition at the bias (bg1, ba1) (ImuTypes.cc:289-312): FP32 like the reference
__device__ void imu_delta(const morb_imu_preintegrated& P, const double* bg1, const double* ba1, double* dR, double* dV, double* dP,
                          double* dbg3) {
  const float b1[6] = {(float)ba1[0], (float)ba1[1], (float)ba1[2], (float)bg1[0], (float)bg1[1], (float)bg1[2]};
  const float dbg[3] = {b1[3] - P.b[3], b1[4] - P.b[4], b1[5] - P.b[5]};
  const float dba[3] = {b1[0] - P.b[0], b1[1] - P.b[1], b1[2] - P.b[2]};
  float w[3], W[9], WW[9], E[9], dRf[9];
  mul3v(P.JRg, dbg, w);
  const float t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], t = sqrtf(t2);
  hatf(w, W);
  mul33(W, W, WW);
  if (t < 1e-5f) for (int k = 0; k < 9; ++k) E[k] = ((k & 3) == 0 ? 1.f : 0.f) + W[k] + 0.5f * WW[k];
  else { const float sn = morbm::sinf_glibc(t), cs = morbm::cosf_glibc(t); for (int k = 0; k < 9; ++k) E[k] = ((k & 3) == 0 ? 1.f : 0.f) + W[k] * sn / t + WW[k] * (1.0f - cs) / t2; }
  mul33(P.dR, E, dRf);
  normalize_rotation_f(dRf);
  for (int k = 0; k < 9; ++k) dR[k] = dRf[k];
  float g1[3], a1[3];
  mul3v(P.JVg, dbg, g1); mul3v(P.JVa, dba, a1);
  for (int k = 0; k < 3; ++k) dV[k] = (double)(P.dV[k] + g1[k] + a1[k]);
  mul3v(P.JPg, dbg, g1); mul3v(P.JPa, dba, a1);
  for (int k = 0; k < 3; ++k) dP[k] = (double)(P.dP[k] + g1[k] + a1[k]);
  for (int k = 0; k < 3; ++k) dbg3[k] = dbg[k];
}
// EdgeInertial between state 1 (S1) and state 2 (S2): error and, when J != nullptr, the 9 x 24 Jacobian (edge column order
// P1 V1 G1 A1 P2 V2) written to LDS.  G2oTypes.cc:494-585.  One thread.
// delta != nullptr: dR dV dP dbg precomputed (state 1 fixed).  full == false: only the (P2, V2) column blocks are written.
// J must have been zeroed once: the same entries are rewritten at every call.
__device__ void inertial_edge(const morb_imu_preintegrated& P, const VIState& S1, const VIState& S2, const double* delta, bool full,
                              double* err, double* J) {
  double dR[9], dV[3], dP[3], dbg[3];
  if (delta) {
    for (int k = 0; k < 9; ++k) dR[k] = delta[k];
    for (int k = 0; k < 3; ++k) { dV[k] = delta[9 + k]; dP[k] = delta[12 + k]; dbg[k] = delta[15 + k]; }
  } else imu_delta(P, S1.bg, S1.ba, dR, dV, dP, dbg);
  const double dt = P.dT;
  double Rbw1[9], dRt[9], M[9], eR[9], er[3];
  transpose33(S1.Rwb, Rbw1);
  transpose33(dR, dRt);
  mul33(dRt, Rbw1, M);
  mul33(M, S2.Rwb, eR);
  log_so3(eR, er);
  const double g[3] = {0, 0, -(double)9.81f};
  double t[3], a1[3], a2[3];
  for (int k = 0; k < 3; ++k) t[k] = S2.v[k] - S1.v[k] - g[k] * dt;
  mul3v(Rbw1, t, a1);
  for (int k = 0; k < 3; ++k) t[k] = S2.twb[k] - S1.twb[k] - S1.v[k] * dt - g[k] * dt * dt / 2;
  mul3v(Rbw1, t, a2);
  for (int k = 0; k < 3; ++k) { err[k] = er[k]; err[3 + k] = a1[k] - dV[k]; err[6 + k] = a2[k] - dP[k]; }
  if (!J) return;
  double invJr[9], T[9], T2[9], W[9];
  inv_right_jacobian_so3(er, invJr);
  // pose 2, velocity 2
  put33(J, 24, 0, 15, invJr, 1.0);
  mul33(Rbw1, S2.Rwb, T);
  put33(J, 24, 6, 18, T, 1.0);
  put33(J, 24, 3, 21, Rbw1, 1.0);
  if (!full) return;
  // pose 1
  transpose33(S2.Rwb, T2);
  mul33(invJr, T2, T); mul33(T, S1.Rwb, T2);
  put33(J, 24, 0, 0, T2, -1.0);
  W[0] = 0; W[1] = -a1[2]; W[2] = a1[1]; W[3] = a1[2]; W[4] = 0; W[5] = -a1[0]; W[6] = -a1[1]; W[7] = a1[0]; W[8] = 0;
  put33(J, 24, 3, 0, W, 1.0);
  {
    double a3[3];
    for (int k = 0; k < 3; ++k) t[k] = S2.twb[k] - S1.twb[k] - S1.v[k] * dt - 0.5 * g[k] * dt * dt;
    mul3v(Rbw1, t, a3);
    W[0] = 0; W[1] = -a3[2]; W[2] = a3[1]; W[3] = a3[2]; W[4] = 0; W[5] = -a3[0]; W[6] = -a3[1]; W[7] = a3[0]; W[8] = 0;
    put33(J, 24, 6, 0, W, 1.0);
  }
  for (int k = 0; k < 3; ++k) J[(6 + k) * 24 + 3 + k] = -1.0;
  // velocity 1
  put33(J, 24, 3, 6, Rbw1, -1.0);
  for (int k = 0; k < 9; ++k) T[k] = Rbw1[k] * dt;
  put33(J, 24, 6, 6, T, -1.0);
  // gyro bias 1
  {
    double JRg[9], w3[3], rj[9], eRt[9];
    for (int k = 0; k < 9; ++k) JRg[k] = P.JRg[k];
    mul3v(JRg, dbg, w3);
    right_jacobian_so3(w3, rj);
    transpose33(eR, eRt);
    mul33(invJr, eRt, T); mul33(T, rj, T2); mul33(T2, JRg, T);
    put33(J, 24, 0, 9, T, -1.0);
    for (int k = 0; k < 9; ++k) T[k] = P.JVg[k];
    put33(J, 24, 3, 9, T, -1.0);
    for (int k = 0; k < 9; ++k) T[k] = P.JPg[k];
    put33(J, 24, 6, 9, T, -1.0);
  }
  // acc bias 1
  for (int k = 0; k < 9; ++k) T[k] = P.JVa[k];
  put33(J, 24, 3, 12, T, -1.0);
  for (int k = 0; k < 9; ++k) T[k] = P.JPa[k];
  put33(J, 24, 6, 12, T, -1.0);
}

// ImuCamPose's constant part: Tcb = Tbc^-1 and, on a fisheye rig, the right camera behind Trl (G2oTypes.cc:96-113).
// rig28 = left KB8 (8), right KB8 (8), Trl rotation (9, row-major) + translation (3), or NULL for one pinhole camera.
inline void make_geom(const float* Tbc12, float fx, float fy, float cx, float cy, float bf, const float* rig28, CamGeom& g) {
  memset(&g, 0, sizeof g);
  for (int k = 0; k < 9; ++k) g.Rbc[k] = Tbc12[k];
  for (int k = 0; k < 3; ++k) g.tbc[k] = Tbc12[9 + k];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) g.Rcb[r * 3 + c] = g.Rbc[c * 3 + r];   // mTcb = mTbc.inverse()
  for (int r = 0; r < 3; ++r) g.tcb[r] = -(g.Rcb[r * 3] * g.tbc[0] + g.Rcb[r * 3 + 1] * g.tbc[1] + g.Rcb[r * 3 + 2] * g.tbc[2]);
  g.bf = bf; g.fx = fx; g.fy = fy; g.cx = cx; g.cy = cy;
  if (!rig28) return;
  g.rig = 1;
  memcpy(g.kb[0], rig28, 32); memcpy(g.kb[1], rig28 + 8, 32);
  double Rrl[9], trl[3];
  for (int k = 0; k < 9; ++k) Rrl[k] = rig28[16 + k];
  for (int k = 0; k < 3; ++k) trl[k] = rig28[25 + k];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) g.Rcb1[r * 3 + c] = Rrl[r * 3] * g.Rcb[c] + Rrl[r * 3 + 1] * g.Rcb[3 + c] + Rrl[r * 3 + 2] * g.Rcb[6 + c];
    g.tcb1[r] = Rrl[r * 3] * g.tcb[0] + Rrl[r * 3 + 1] * g.tcb[1] + Rrl[r * 3 + 2] * g.tcb[2] + trl[r];
  }
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) g.Rbc1[r * 3 + c] = g.Rcb1[c * 3 + r];
  for (int r = 0; r < 3; ++r) g.tbc1[r] = -(g.Rbc1[r * 3] * g.tcb1[0] + g.Rbc1[r * 3 + 1] * g.tcb1[1] + g.Rbc1[r * 3 + 2] * g.tcb1[2]);
}

}  // namespace
