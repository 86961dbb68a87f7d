// Device helpers PoseOptimization (optimizer.hip) and LocalBundleAdjustment (local_ba.hip) share: the SE3Quat algebra, the reference's
// projection edge with its pose Jacobian, the fixed-order block sum and the fisheye rig (Huber's kernel: quat_huber.h).  What only one of the two
// uses lives in that unit; the binary edges at the end (point Jacobian, pinhole or rig) serve the bundle adjusters of local_ba.hip and
// global_ba.hip.  Everything is in an unnamed namespace: each unit gets its own copy, and the kernels keep their mangled names.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "morb/camera_math.h"
#include "quat_huber.h"
#include "wave.h"

namespace {

struct Cam { float fx, fy, cx, cy, bf; };

struct SE3 {
  double q[4];  // x y z w
  double t[3];
};

// ---- SE3Quat algebra (g2o/types/se3quat.h; Eigen quaternion formulas) ---------------------------------------
__device__ __forceinline__ void se3_normalize(SE3& s) {
  if (s.q[3] < 0) { s.q[0] = -s.q[0]; s.q[1] = -s.q[1]; s.q[2] = -s.q[2]; s.q[3] = -s.q[3]; }
  const double n = sqrt(s.q[0] * s.q[0] + s.q[1] * s.q[1] + s.q[2] * s.q[2] + s.q[3] * s.q[3]);
  s.q[0] /= n; s.q[1] /= n; s.q[2] /= n; s.q[3] /= n;
}
__device__ __forceinline__ void se3_map(const SE3& T, const double* x, double* out) {
  q_rotate(T.q, x, out);
  out[0] += T.t[0]; out[1] += T.t[1]; out[2] += T.t[2];
}
__device__ __forceinline__ void q_to_R(const double* q, double* R) {
  const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
// Eigen's matrix -> quaternion (Quaternion.h, QuaternionBase::operator=(MatrixBase)); the largest-diagonal branch indexes the matrix with
// i, j = (i + 1) % 3, k = (j + 1) % 3 — as run-time indices they put the matrix into scratch memory in every pose update (a store and nine
// dependent loads on the critical path of each LM trial), so the three cases are spelled out with constant indices.
template <int I, int J, int K>
__device__ __forceinline__ void R_to_q_case(const double* m, double* q) {
  double t = sqrt(m[I * 3 + I] - m[J * 3 + J] - m[K * 3 + K] + 1.0);
  q[I] = 0.5 * t;
  t = 0.5 / t;
  q[3] = (m[K * 3 + J] - m[J * 3 + K]) * t;
  q[J] = (m[J * 3 + I] + m[I * 3 + J]) * t;
  q[K] = (m[K * 3 + I] + m[I * 3 + K]) * t;
}
__device__ __forceinline__ void R_to_q(const double* m, double* q) {
  double t = m[0] + m[4] + m[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
  } else {
    const bool one = m[4] > m[0];
    const bool two = m[8] > (one ? m[4] : m[0]);
    if (two) R_to_q_case<2, 0, 1>(m, q);
    else if (one) R_to_q_case<1, 2, 0>(m, q);
    else R_to_q_case<0, 1, 2>(m, q);
  }
}
__device__ __forceinline__ SE3 se3_mul(const SE3& a, const SE3& b) {
  SE3 r = a;
  double rt[3];
  q_rotate(a.q, b.t, rt);
  r.t[0] += rt[0]; r.t[1] += rt[1]; r.t[2] += rt[2];
  const double* p = a.q; const double* o = b.q;
  r.q[3] = p[3] * o[3] - p[0] * o[0] - p[1] * o[1] - p[2] * o[2];
  r.q[0] = p[3] * o[0] + p[0] * o[3] + p[1] * o[2] - p[2] * o[1];
  r.q[1] = p[3] * o[1] + p[1] * o[3] + p[2] * o[0] - p[0] * o[2];
  r.q[2] = p[3] * o[2] + p[2] * o[3] + p[0] * o[1] - p[1] * o[0];
  se3_normalize(r);
  return r;
}
// glibc's sin for |x| < 0.126 (sysdeps/ieee754/dbl-64/s_sin.c: TAYLOR_SIN, 0.501 ulp; |x| < 2^-26: x): the argument range of an LM update's rotation.
// Larger arguments fall back to the device library's sin (<= 1 ulp from it).
__device__ __forceinline__ double sin_glibc_small(double x) {
  const double ax = fabs(x);
  if (ax < 0x1p-26) return x;
  if (ax < 0.126) {
    const double s1 = -0x1.5555555555555p-3, s2 = 0x1.1111111110ECEp-7, s3 = -0x1.A01A019DB08B8p-13, s4 = 0x1.71DE27B9A7ED9p-19, s5 = -0x1.ADDFFC2FCDF59p-26;
    const double xx = x * x;
    const double poly = ((((s5 * xx + s4) * xx + s3) * xx + s2) * xx) + s1;
    const double t = (poly * x - 0.5 * 0.0) * xx + 0.0;   // TAYLOR_SIN(xx, a, da) with da = 0
    return x + t;
  }
  return sin(x);
}
__device__ __forceinline__ SE3 se3_exp(const double* u) {
  const double wx = u[0], wy = u[1], wz = u[2];
  const double theta = sqrt(wx * wx + wy * wy + wz * wz);
  const double Om[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
  double Om2[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Om2[i * 3 + j] = Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j] + Om[i * 3 + 2] * Om[6 + j];
  double R[9], V[9];
  if (theta < 0.00001) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { R[i] = (i % 4 == 0 ? 1.0 : 0.0) + Om[i] + Om2[i]; V[i] = R[i]; }
  } else {
    const double s = sin_glibc_small(theta), c = cos(theta);
    const double a = s / theta, b = (1 - c) / (theta * theta), cc = (theta - s) / cube_rn(theta);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      R[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * Om[i] + b * Om2[i];
      V[i] = (i % 4 == 0 ? 1.0 : 0.0) + b * Om[i] + cc * Om2[i];
    }
  }
  SE3 r;
  R_to_q(R, r.q);
  for (int i = 0; i < 3; ++i) r.t[i] = V[i * 3] * u[3] + V[i * 3 + 1] * u[4] + V[i * 3 + 2] * u[5];
  se3_normalize(r);
  return r;
}
__device__ __forceinline__ SE3 se3_from_float(const float* p) {
  SE3 s;
  for (int i = 0; i < 4; ++i) s.q[i] = (double)p[i];
  for (int i = 0; i < 3; ++i) s.t[i] = (double)p[4 + i];
  se3_normalize(s);
  return s;
}

// ---- edges -------------------------------------------------------------------------------------------------
// error = obs - project(xc); stereo = (ur >= 0).  Returns chi2 = info * |err|^2 (information = info * I).
__device__ __forceinline__ double edge_error(const Cam& cam, bool stereo, const double* xc, const float* obs, double info,
                                             double* err) {
  if (!stereo) {  // Pinhole::project(Vector3d) (Pinhole.cpp:38-44)
    err[0] = (double)obs[0] - ((double)cam.fx * xc[0] / xc[2] + (double)cam.cx);
    err[1] = (double)obs[1] - ((double)cam.fy * xc[1] / xc[2] + (double)cam.cy);
    err[2] = 0;
    return err[0] * (info * err[0]) + err[1] * (info * err[1]);
  }
  const float invz = (float)(1.0 / xc[2]);  // cam_project: `const float invz` (types_six_dof_expmap.cpp:191,340)
  const double p0 = xc[0] * invz * (double)cam.fx + (double)cam.cx;
  const double p1 = xc[1] * invz * (double)cam.fy + (double)cam.cy;
  const double p2 = p0 - (double)cam.bf * invz;
  err[0] = (double)obs[0] - p0; err[1] = (double)obs[1] - p1; err[2] = (double)obs[2] - p2;
  return err[0] * (info * err[0]) + err[1] * (info * err[1]) + err[2] * (info * err[2]);
}
// pose Jacobian (d x 6); unary = the "...OnlyPose" formulas
__device__ __forceinline__ void jac_pose(const Cam& cam, bool stereo, bool unary, const double* xc, double* Jp) {
  const double x = xc[0], y = xc[1], z = xc[2];
  const double fx = cam.fx, fy = cam.fy, bf = cam.bf;
  if (!stereo) {  // -projectJac * SE3deriv (OptimizableTypes.cpp:49-62 / :134-156)
    const double a = fx / z, b = -fx * x / (z * z), c = fy / z, d = -fy * y / (z * z);
    Jp[0] = -(b * y); Jp[1] = -(a * z + b * -x); Jp[2] = -(a * -y); Jp[3] = -a; Jp[4] = -0.0; Jp[5] = -b;
    Jp[6] = -(c * -z + d * y); Jp[7] = -(d * -x); Jp[8] = -(c * x); Jp[9] = -0.0; Jp[10] = -c; Jp[11] = -d;
    for (int i = 12; i < 18; ++i) Jp[i] = 0;
  } else if (unary) {  // EdgeStereoSE3ProjectXYZOnlyPose::linearizeOplus (:375-403)
    const double invz = 1.0 / z, invz_2 = invz * invz;
    Jp[0] = x * y * invz_2 * fx; Jp[1] = -(1 + (x * x * invz_2)) * fx; Jp[2] = y * invz * fx;
    Jp[3] = -invz * fx; Jp[4] = 0; Jp[5] = x * invz_2 * fx;
    Jp[6] = (1 + y * y * invz_2) * fy; Jp[7] = -x * y * invz_2 * fy; Jp[8] = -x * invz * fy;
    Jp[9] = 0; Jp[10] = -invz * fy; Jp[11] = y * invz_2 * fy;
    Jp[12] = Jp[0] - bf * y * invz_2; Jp[13] = Jp[1] + bf * x * invz_2; Jp[14] = Jp[2];
    Jp[15] = Jp[3]; Jp[16] = 0; Jp[17] = Jp[5] - bf * invz_2;
  } else {  // EdgeStereoSE3ProjectXYZ::linearizeOplus (:228-270)
    const double z_2 = z * z;
    Jp[0] = x * y / z_2 * fx; Jp[1] = -(1 + (x * x / z_2)) * fx; Jp[2] = y / z * fx;
    Jp[3] = -1. / z * fx; Jp[4] = 0; Jp[5] = x / z_2 * fx;
    Jp[6] = (1 + y * y / z_2) * fy; Jp[7] = -x * y / z_2 * fy; Jp[8] = -x / z * fy;
    Jp[9] = 0; Jp[10] = -1. / z * fy; Jp[11] = y / z_2 * fy;
    Jp[12] = Jp[0] - bf * y / z_2; Jp[13] = Jp[1] + bf * x / z_2; Jp[14] = Jp[2];
    Jp[15] = Jp[3]; Jp[16] = 0; Jp[17] = Jp[5] - bf / z_2;
  }
}

// ---- block reductions (fixed order -> deterministic) --------------------------------------------------------
__device__ __forceinline__ double wave_sum_d(double v) { return morbwave::sum_f64(v); }   // DPP (wave.h), all lanes active
template <int NW>
__device__ __forceinline__ double block_sum_d(double v, double* red /*[NW]*/) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) s += red[i];
  return s;
}

// ---- KannalaBrandt8 (fisheye) camera in the optimisers (KannalaBrandt8.cpp:48-66, :149-184) ------------------
struct Rig {            // fisheye stereo rig: left / right KB8 cameras and mTrl (left-camera frame -> right-camera frame)
  float kbL[8], kbR[8];
  SE3 Trl;
};

// the fisheye rig of a call: KB8 cameras and Trl7 = (qx, qy, qz, qw, tx, ty, tz)
inline Rig make_rig(const float* camL8, const float* camR8, const float* Trl7) {
  Rig rig;
  memcpy(rig.kbL, camL8, 32);
  memcpy(rig.kbR, camR8, 32);
  {  // g2o::SE3Quat(Trl.unit_quaternion().cast<double>(), Trl.translation().cast<double>()) incl. normalisation
    double q[4] = {Trl7[0], Trl7[1], Trl7[2], Trl7[3]};
    if (q[3] < 0) for (double& c : q) c = -c;
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) rig.Trl.q[i] = q[i] / n;
    for (int i = 0; i < 3; ++i) rig.Trl.t[i] = Trl7[4 + i];
  }
  return rig;
}

// point Jacobian (d x 3)
__device__ __forceinline__ void jac_point(const Cam& cam, bool stereo, const double* xc, const double* R, double* Jl) {
  const double x = xc[0], y = xc[1], z = xc[2];
  const double fx = cam.fx, fy = cam.fy, bf = cam.bf;
  if (!stereo) {  // -projectJac * R
    const double a = fx / z, b = -fx * x / (z * z), c = fy / z, d = -fy * y / (z * z);
    for (int k = 0; k < 3; ++k) { Jl[k] = -(a * R[k] + b * R[6 + k]); Jl[3 + k] = -(c * R[3 + k] + d * R[6 + k]); Jl[6 + k] = 0; }
  } else {
    const double z_2 = z * z;
    for (int k = 0; k < 3; ++k) {
      Jl[k] = -fx * R[k] / z + fx * x * R[6 + k] / z_2;
      Jl[3 + k] = -fy * R[3 + k] / z + fy * y * R[6 + k] / z_2;
      Jl[6 + k] = Jl[k] - bf * R[6 + k] / z_2;
    }
  }
}

// ---- binary edges of the bundle adjusters (local_ba.hip, global_ba.hip), pinhole or fisheye rig -------------------------
// obs[2] >= 0: EdgeStereoSE3ProjectXYZ; -1: EdgeSE3ProjectXYZ with the pinhole camera; -2: EdgeSE3ProjectXYZ with the
// left KB8 camera; -3: EdgeSE3ProjectXYZToBody (right KB8 camera behind mTrl).  (Optimizer.cc:1244-1351)
__device__ __forceinline__ bool edge_is_kb8(const Rig* rig, const float* o) { return rig != nullptr && o[2] < -1.5f; }
__device__ __forceinline__ double ba_edge_error(const Cam& cam, const Rig* rig, bool st, const double* xc, const float* o,
                                                double info, double* err) {
  if (!edge_is_kb8(rig, o)) return edge_error(cam, st, xc, o, info, err);
  double uv[2];
  if (o[2] > -2.5f) morbcam::kb8_project_d(rig->kbL, xc, uv);
  else { double xr[3]; se3_map(rig->Trl, xc, xr); morbcam::kb8_project_d(rig->kbR, xr, uv); }   // (mTrl * T).map(Xw) = mTrl.map(T.map(Xw))
  err[0] = (double)o[0] - uv[0]; err[1] = (double)o[1] - uv[1]; err[2] = 0;
  return err[0] * (info * err[0]) + err[1] * (info * err[1]);
}
// Jp (d x 6) and / or Jl (d x 3); R = rotation of the keyframe pose.  OptimizableTypes.cpp:134-156 / :185-208
// RIG = false: the problem has no fisheye rig.  The KannalaBrandt8 branch (its float libm, the right camera's extrinsics) otherwise costs
// the pinhole build kernel 100 VGPRs (220 instead of 119) and puts the pose Jacobian into scratch memory — for a branch it never takes.
template <bool RIG>
__device__ __forceinline__ void ba_edge_jac(const Cam& cam, const Rig* rig, bool st, const double* xc, const float* o,
                                            const double* R, double* Jp, double* Jl) {
  // RIG = true: EVERY edge of the problem is a KannalaBrandt8 edge (morb_ba_problem_create_fisheye writes obs[2] = -2 / -3 for all of them),
  // so the choice is made at compile time: with a run-time `edge_is_kb8` both branches wrote Jp and the array went to scratch memory (160 B)
  if (!RIG) {
    if (Jp) jac_pose(cam, st, false, xc, Jp);
    if (Jl) jac_point(cam, st, xc, R, Jl);
    return;
  }
  const double x = xc[0], y = xc[1], z = xc[2];
  double pj[6], pjM[6];
  if (o[2] > -2.5f) {
    morbcam::kb8_project_jac(rig->kbL, xc, pj);
    _Pragma("unroll") for (int k = 0; k < 6; ++k) pjM[k] = pj[k];
  } else {
    double xr[3], M[9];
    se3_map(rig->Trl, xc, xr);
    morbcam::kb8_project_jac(rig->kbR, xr, pj);
    q_to_R(rig->Trl.q, M);
    _Pragma("unroll") for (int r = 0; r < 2; ++r)
      _Pragma("unroll") for (int c = 0; c < 3; ++c) pjM[r * 3 + c] = pj[r * 3] * M[c] + pj[r * 3 + 1] * M[3 + c] + pj[r * 3 + 2] * M[6 + c];
  }
  _Pragma("unroll") for (int r = 0; r < 2; ++r) {
    const double a = pjM[r * 3], b = pjM[r * 3 + 1], c = pjM[r * 3 + 2];
    if (Jp) {
      Jp[r * 6 + 0] = -(b * -z + c * y); Jp[r * 6 + 1] = -(a * z + c * -x); Jp[r * 6 + 2] = -(a * -y + b * x);
      Jp[r * 6 + 3] = -a; Jp[r * 6 + 4] = -b; Jp[r * 6 + 5] = -c;
    }
    if (Jl) _Pragma("unroll") for (int k = 0; k < 3; ++k) Jl[r * 3 + k] = -(a * R[k] + b * R[3 + k] + c * R[6 + k]);
  }
  if (Jp) _Pragma("unroll") for (int k = 12; k < 18; ++k) Jp[k] = 0;
  if (Jl) _Pragma("unroll") for (int k = 6; k < 9; ++k) Jl[k] = 0;
}
// isDepthPositive (OptimizableTypes.h:117-123 / :152-158)
__device__ __forceinline__ bool ba_depth_positive(const Rig* rig, const float* o, const double* xc) {
  if (edge_is_kb8(rig, o) && !(o[2] > -2.5f)) { double xr[3]; se3_map(rig->Trl, xc, xr); return xr[2] > 0.0; }
  return xc[2] > 0.0;
}

}  // namespace
