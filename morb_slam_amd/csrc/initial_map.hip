// The numeric rest of Tracking::CreateInitialMapMonocular (reference src/Tracking.cc:2345-2430) for MI355X (gfx950), batched: the bundle
// adjustment of the two new keyframes and their points (Optimizer::GlobalBundleAdjustemnt -> BundleAdjustment, src/Optimizer.cc:47-362),
// KeyFrame::ComputeSceneMedianDepth(2) (src/KeyFrame.cc:796-826), the reset test, the rescaling to unit median depth and
// MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:464-519).
//   k_initial_map — one workgroup per frame pair, everything in ONE launch on the caller's stream.
// The graph: keyframe 1 fixed at the identity, keyframe 2 free, every point seen by both through one EdgeSE3ProjectXYZ each.  The reduced
// camera system is therefore ONE 6 x 6 block and the Schur complement a sum over the points:
//   * the points of a problem are compacted in keypoint order (ballot + running offset) into records of IM_RS doubles, in LDS up to
//     IM_LDS_N keypoints per frame, else in the handle's workspace; a thread owns the points tid, tid + IM_T, ...: no bound but cap;
//   * build: per point the two edges, Hll (upper triangle), bl, Hpl; the 21 + 6 values of Hpp and bp are summed per thread in point
//     order, per wave on the DPP path, the four waves in order: no atomics, two runs give the same bits;
//   * trial: per point Dinv = (Hll + lambda I)^-1 and its 27 Schur terms, summed the same way; EVERY thread then factorises the 6 x 6
//     system (LDL^T, a zero or NaN pivot fails, as in LocalBundleAdjustment) in registers: no broadcast, no barrier; back-substitution,
//     oplus and the trial state's chi2 per point in one pass;
//   * the LM decisions are csrc/lm_control.h's; computeLambdaInit takes the maximum over the diagonals of Hpp and every Hll.
// FP64 like g2o; the reference's float leaks (float camera parameters, information and Huber delta, KannalaBrandt8::project's float atan2f)
// are reproduced as LocalBundleAdjustment reproduces them.  The mono edge is restated here on include/morb/camera_math.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.h"
#include "handles.h"
#include "lm_control.h"
#include "morb/camera_math.h"
#include "morb/initial_map_math.h"
#include "optimizer_device.h"
#include "wave.h"

using namespace morb;

namespace {

constexpr int IM_T = 256, IM_W = IM_T / 64;
constexpr int IM_LDS_N = 512;   // the records of a problem stay in LDS up to this cap: 512 * IM_RS * 8 B = 148 KB beside 1 KB of static LDS
// per-point record (doubles): X 3 | backup 3 | Hll upper triangle 6 | bl 3 | Hpl 6 x 3 | eight 32-bit words: obs1 2, obs2 2, info1, info2 (float),
// keypoint 1, keypoint 2 (int).  The odd stride spreads consecutive records over the LDS banks.  After the solve bl[0] holds the depth key.
constexpr int IM_X = 0, IM_XBK = 3, IM_HLL = 6, IM_BL = 12, IM_HPL = 15, IM_WORDS = 33, IM_RS = 37;
constexpr int IM_NR = 27;       // the sums of a pass: 21 of the 6 x 6 upper triangle (rows first), 6 of the right-hand side

struct ImShared {
  double part[IM_W][IM_NR + 1];
  int ipart[IM_W];
  int flag;
};

struct ImArgs {
  morb_frame_params P;
  float cam[8];
  int cap;
  const int *img1, *img2, *count;
  const morb_keypoint* kps;
  const int* matches12;
  const int* ok;
  const float *T21, *P3D;
  const uint8_t* triangulated;
  int nIterations, robust;
  float depthScale;
  int minTracked;
  const unsigned char* stop;
  int* status;
  float *Tcw2, *mpPos, *mpNormal, *mpDist;
  uint8_t* hasMP;
  int* stats;
  double* chi2;
  float* median;
  double* ws;
};

// Eigen's matrix -> quaternion in float (Sophus::SE3f::unit_quaternion of the pose KeyFrame::SetPose received); constant indices as R_to_q has them
template <int I, int J, int K>
__device__ __forceinline__ void im_R_to_q_case(const float* m, float* q) {
  float t = sqrtf(m[I * 3 + I] - m[J * 3 + J] - m[K * 3 + K] + 1.0f);
  q[I] = 0.5f * t;
  t = 0.5f / t;
  q[3] = (m[K * 3 + J] - m[J * 3 + K]) * t;
  q[J] = (m[J * 3 + I] + m[I * 3 + J]) * t;
  q[K] = (m[K * 3 + I] + m[I * 3 + K]) * t;
}
__device__ __forceinline__ void im_R_to_q(const float* m, float* q) {
  float t = m[0] + m[4] + m[8];
  if (t > 0) {
    t = sqrtf(t + 1.0f);
    q[3] = 0.5f * t;
    t = 0.5f / t;
    q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
  } else {
    const bool one = m[4] > m[0];
    const bool two = m[8] > (one ? m[4] : m[0]);
    if (two) im_R_to_q_case<2, 0, 1>(m, q);
    else if (one) im_R_to_q_case<1, 2, 0>(m, q);
    else im_R_to_q_case<0, 1, 2>(m, q);
  }
}
// Sophus::SE3f(SE3quat.rotation().cast<float>(), SE3quat.translation().cast<float>()) as R (9, row-major) then t (Optimizer.cc:286-287)
__device__ __forceinline__ void im_pose_to_float(const SE3& T, float* out12) {
  float q[4] = {(float)T.q[0], (float)T.q[1], (float)T.q[2], (float)T.q[3]};
  const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; ++i) q[i] /= n;
  const float tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
  const float twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const float txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const float tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  out12[0] = 1 - (tyy + tzz); out12[1] = txy - twz; out12[2] = txz + twy;
  out12[3] = txy + twz; out12[4] = 1 - (txx + tzz); out12[5] = tyz - twx;
  out12[6] = txz - twy; out12[7] = tyz + twx; out12[8] = 1 - (txx + tyy);
  for (int i = 0; i < 3; ++i) out12[9 + i] = (float)T.t[i];
}

// EdgeSE3ProjectXYZ::computeError (OptimizableTypes.h:96-101): obs - pCamera->project(xc); Pinhole::project(Vector3d) (Pinhole.cpp:38-44) with its
// float parameters, KannalaBrandt8::project(Vector3d) from camera_math.h
template <bool KB8>
__device__ __forceinline__ void im_edge_error(const float* c, const double* xc, float ox, float oy, double* err) {
  double uv[2];
  if (KB8) morbcam::kb8_project_d(c, xc, uv);
  else {
    uv[0] = (double)c[0] * xc[0] / xc[2] + (double)c[2];
    uv[1] = (double)c[1] * xc[1] / xc[2] + (double)c[3];
  }
  err[0] = (double)ox - uv[0];
  err[1] = (double)oy - uv[1];
}
// pCamera->projectJac(xc) (2 x 3): Pinhole.cpp:65-76, KannalaBrandt8.cpp:164-199
template <bool KB8>
__device__ __forceinline__ void im_project_jac(const float* c, const double* xc, double* pj) {
  if (KB8) { morbcam::kb8_project_jac(c, xc, pj); return; }
  const double fx = c[0], fy = c[1], z = xc[2];
  pj[0] = fx / z; pj[1] = 0.0; pj[2] = -fx * xc[0] / (z * z);
  pj[3] = 0.0; pj[4] = fy / z; pj[5] = -fy * xc[1] / (z * z);
}
// linearizeOplus (OptimizableTypes.cpp:134-156): Jl = -projectJac * R (2 x 3), Jp = -projectJac * [-[xc]x | I] (2 x 6); a null pointer skips the block
__device__ __forceinline__ void im_edge_jac(const double* pj, const double* xc, const double* R, double* Jp, double* Jl) {
  const double x = xc[0], y = xc[1], z = xc[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const double a = pj[r * 3], b = pj[r * 3 + 1], c = pj[r * 3 + 2];
    if (Jp) {
      Jp[r * 6 + 0] = -(b * -z + c * y); Jp[r * 6 + 1] = -(a * z + c * -x); Jp[r * 6 + 2] = -(a * -y + b * x);
      Jp[r * 6 + 3] = -a; Jp[r * 6 + 4] = -b; Jp[r * 6 + 5] = -c;
    }
    if (R) {
#pragma unroll
      for (int k = 0; k < 3; ++k) Jl[r * 3 + k] = -(a * R[k] + b * R[3 + k] + c * R[6 + k]);
    } else {   // keyframe 1: the identity
      Jl[r * 3] = -a; Jl[r * 3 + 1] = -b; Jl[r * 3 + 2] = -c;
    }
  }
}
// inverse of the symmetric 3 x 3 whose upper triangle is h (00 01 02 11 12 22): the cofactor form LocalBundleAdjustment uses on the full matrix
__device__ __forceinline__ void im_inv3_sym(const double* h, double lambda, double* o) {
  const double m0 = h[0] + lambda, m1 = h[1], m2 = h[2], m4 = h[3] + lambda, m5 = h[4], m8 = h[5] + lambda;
  const double c00 = m4 * m8 - m5 * m5, c01 = m5 * m2 - m1 * m8, c02 = m1 * m5 - m4 * m2;
  const double id = 1.0 / (m0 * c00 + m1 * c01 + m2 * c02);
  o[0] = c00 * id; o[1] = (m2 * m5 - m1 * m8) * id; o[2] = (m1 * m5 - m2 * m4) * id;
  o[3] = c01 * id; o[4] = (m0 * m8 - m2 * m2) * id; o[5] = (m2 * m1 - m0 * m5) * id;
  o[6] = c02 * id; o[7] = (m1 * m2 - m0 * m5) * id; o[8] = (m0 * m4 - m1 * m1) * id;
}

// the 6 x 6 reduced system in registers: A (upper triangle by rows, 21) and b -> x; right-looking LDL^T with LocalBundleAdjustment's pivot rule
// (a pivot that is zero or NaN fails).  Every index is a constant once the loops are unrolled.
__device__ __forceinline__ bool im_solve6(const double* up, const double* rhs, double* x) {
  double A[36];
  {
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) { A[r * 6 + c] = up[q]; A[c * 6 + r] = up[q]; ++q; }
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double d = A[j * 6 + j];
    if (d == 0 || d != d) ok = false;
#pragma unroll
    for (int i = j + 1; i < 6; ++i)
#pragma unroll
      for (int k = j + 1; k <= i; ++k) A[i * 6 + k] -= A[i * 6 + j] * A[k * 6 + j] / d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) A[i * 6 + j] /= d;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = rhs[i];
#pragma unroll
  for (int j = 0; j < 6; ++j)
#pragma unroll
    for (int i = j + 1; i < 6; ++i) x[i] -= A[i * 6 + j] * x[j];
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] /= A[i * 6 + i];
#pragma unroll
  for (int j = 5; j >= 0; --j)
#pragma unroll
    for (int i = 0; i < j; ++i) x[i] -= A[j * 6 + i] * x[j];
  return ok;
}

// robust chi2 of one point's two edges at X under the pose S of keyframe 2 (keyframe 1 sees X itself); wf = the record's words
template <bool KB8>
__device__ __forceinline__ double im_point_chi2(const float* cam, bool robust, double delta, const float* wf, const double* X, const SE3& S) {
  double xc[3], e[2], w;
  im_edge_error<KB8>(cam, X, wf[0], wf[1], e);
  const double i1d = (double)wf[4], i2d = (double)wf[5];
  double c = e[0] * (i1d * e[0]) + e[1] * (i1d * e[1]);
  double s = robust ? huber(delta, c, &w) : c;
  se3_map(S, X, xc);
  im_edge_error<KB8>(cam, xc, wf[2], wf[3], e);
  c = e[0] * (i2d * e[0]) + e[1] * (i2d * e[1]);
  s += robust ? huber(delta, c, &w) : c;
  return s;
}

// sums of K values over the workgroup, in a fixed order: per thread (its points in order), per wave (DPP), the waves in order
template <int K>
__device__ __forceinline__ void im_reduce(double* acc, ImShared& sh, int lane, int wv) {
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double s = morbwave::sum_f64(acc[k]);
    if (lane == 0) sh.part[wv][k] = s;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = ((sh.part[0][k] + sh.part[1][k]) + sh.part[2][k]) + sh.part[3][k];
}

// KB8: the camera model of both keyframes; GWS: the records live in the global workspace (cap > IM_LDS_N) instead of LDS
template <bool KB8, bool GWS>
__global__ __launch_bounds__(IM_T) void k_initial_map(const ImArgs a) {
  __shared__ ImShared sh;
  extern __shared__ __align__(16) double sRec[];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int cap = a.cap;
  double* const rec = GWS ? a.ws + (size_t)p * cap * IM_RS : sRec;
  float* const mpPos = a.mpPos + (size_t)p * cap * 3;
  float* const mpNormal = a.mpNormal + (size_t)p * cap * 3;
  float* const mpDist = a.mpDist + (size_t)p * cap * 2;
  uint8_t* const hasMP = a.hasMP + (size_t)p * cap;

  // ---- every output row of the problem starts at zero
  for (int i = tid; i < cap * 3; i += IM_T) { mpPos[i] = 0.f; mpNormal[i] = 0.f; }
  for (int i = tid; i < cap * 2; i += IM_T) mpDist[i] = 0.f;
  for (int i = tid; i < cap; i += IM_T) hasMP[i] = 0;
  if (tid < 12) a.Tcw2[12 * p + tid] = 0.f;
  if (a.ok[p] == 0) {   // (uniform) TwoViewReconstruction had returned false: MonocularInitialization does not come here
    if (tid == 0) {
      a.status[p] = morbim::IM_NOT_RUN;
      for (int k = 0; k < 4; ++k) a.stats[4 * p + k] = 0;
      a.chi2[2 * p] = 0.0; a.chi2[2 * p + 1] = 0.0;
      a.median[p] = 0.f;
    }
    return;
  }
  __syncthreads();   // the zeros above are behind the point rows written below

  // ---- the points: frame-1 keypoints with a match in range that was triangulated (Tracking.cc:2318-2323, :2362-2363), in keypoint order
  const int i1 = a.img1[p], i2 = a.img2[p];
  const int n1 = min(a.count[i1], cap), n2 = min(a.count[i2], cap);
  const morb_keypoint* const kp1 = a.kps + (size_t)i1 * cap;
  const morb_keypoint* const kp2 = a.kps + (size_t)i2 * cap;
  int n = 0;
  for (int c0 = 0; c0 < n1; c0 += IM_T) {
    const int i = c0 + tid;
    int j = -1;
    bool f = false;
    if (i < n1) {
      j = a.matches12[(size_t)p * cap + i];
      f = j >= 0 && j < n2 && a.triangulated[(size_t)p * cap + i] != 0;
    }
    const unsigned long long b = __ballot(f);
    if (lane == 0) sh.ipart[wv] = __popcll(b);
    __syncthreads();
    int off = n, tot = 0;
#pragma unroll
    for (int w = 0; w < IM_W; ++w) { if (w < wv) off += sh.ipart[w]; tot += sh.ipart[w]; }
    if (f) {
      double* r = rec + (size_t)(off + __popcll(b & ((1ull << lane) - 1ull))) * IM_RS;
      const float* X = a.P3D + ((size_t)p * cap + i) * 3;
      const morb_keypoint k1 = kp1[i], k2 = kp2[j];
      for (int k = 0; k < 3; ++k) r[IM_X + k] = (double)X[k];   // vPoint->setEstimate(pMP->GetWorldPos().cast<double>())
      float* wf = reinterpret_cast<float*>(r + IM_WORDS);
      int* wi = reinterpret_cast<int*>(r + IM_WORDS);
      wf[0] = k1.x; wf[1] = k1.y; wf[2] = k2.x; wf[3] = k2.y;
      wf[4] = 1.0f / a.P.levelSigma2[k1.octave & 15];            // mvInvLevelSigma2 (ORBextractor.cc:421), as k_pose_edges derives it
      wf[5] = 1.0f / a.P.levelSigma2[k2.octave & 15];
      wi[6] = i; wi[7] = j;
    }
    n += tot;
    __syncthreads();
  }

  // ---- keyframe 2: g2o::SE3Quat(Tcw.unit_quaternion().cast<double>(), Tcw.translation().cast<double>()), every thread its own copy
  SE3 T, Tbk;
  {
    float Rf[9], qf[4];
    for (int k = 0; k < 9; ++k) Rf[k] = a.T21[12 * p + k];
    im_R_to_q(Rf, qf);
    for (int k = 0; k < 4; ++k) T.q[k] = (double)qf[k];
    for (int k = 0; k < 3; ++k) T.t[k] = (double)a.T21[12 * p + 9 + k];
    se3_normalize(T);
    Tbk = T;
  }
  const double delta = (double)(float)sqrt(5.99);   // const float thHuber2D = sqrt(5.99) (Optimizer.cc:126)
  const bool robust = a.robust != 0;
  float cam[8];   // (a copy in registers: a pointer into the argument record sends the whole record to scratch memory)
#pragma unroll
  for (int k = 0; k < 8; ++k) cam[k] = a.cam[k];

  auto stop_set = [&]() -> bool {
    if (!a.stop) return false;
    __syncthreads();
    if (tid == 0) sh.flag = *reinterpret_cast<const volatile unsigned char*>(a.stop + p);   // another stream or the host may set it while this runs
    __syncthreads();
    return sh.flag != 0;
  };
  auto chi2_now = [&]() -> double {
    double s[1] = {0.0};
    for (int q = tid; q < n; q += IM_T) { const double* r = rec + (size_t)q * IM_RS; s[0] += im_point_chi2<KB8>(cam, robust, delta, reinterpret_cast<const float*>(r + IM_WORDS), r + IM_X, T); }
    im_reduce<1>(s, sh, lane, wv);
    return s[0];
  };

  int its = 0, trials = 0, stopSeen = 0;
  const double chiFirst = chi2_now();
  double chiLast = chiFirst;
  if (stop_set()) stopSeen = 1;   // optimize() returns at once: the estimates are the inputs
  else if (n > 0) {
    LmControl c;
    double hpp[IM_NR];   // Hpp (upper triangle by rows) and bp of the current linearisation, in every thread
    for (int iter = 0; iter < a.nIterations; ++iter) {
      if (stop_set()) { stopSeen = 1; break; }
      ++its;
      lm_iteration(c, iter == 0 ? chiFirst : chi2_now());
      // ---- buildSystem
      double R[9];
      q_to_R(T.q, R);
      double md = 0.0;
#pragma unroll
      for (int k = 0; k < IM_NR; ++k) hpp[k] = 0.0;
      for (int q = tid; q < n; q += IM_T) {
        double* r = rec + (size_t)q * IM_RS;
        const float* wf = reinterpret_cast<const float*>(r + IM_WORDS);
        const double X[3] = {r[IM_X], r[IM_X + 1], r[IM_X + 2]};
        double xc[3], e1[2], e2[2], pj[6], Jl1[6], Jl2[6], Jp[12], w1 = 1.0, w2 = 1.0;
        const double i1d = (double)wf[4], i2d = (double)wf[5];
        im_edge_error<KB8>(cam, X, wf[0], wf[1], e1);
        if (robust) huber(delta, e1[0] * (i1d * e1[0]) + e1[1] * (i1d * e1[1]), &w1);
        im_project_jac<KB8>(cam, X, pj);
        im_edge_jac(pj, X, nullptr, nullptr, Jl1);
        se3_map(T, X, xc);
        im_edge_error<KB8>(cam, xc, wf[2], wf[3], e2);
        if (robust) huber(delta, e2[0] * (i2d * e2[0]) + e2[1] * (i2d * e2[1]), &w2);
        im_project_jac<KB8>(cam, xc, pj);
        im_edge_jac(pj, xc, R, Jp, Jl2);
        const double wo1 = w1 * i1d, wo2 = w2 * i2d;
        int u = 0;
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
          r[IM_BL + rr] = (Jl1[rr] * (-i1d * e1[0] * w1) + Jl1[3 + rr] * (-i1d * e1[1] * w1)) + (Jl2[rr] * (-i2d * e2[0] * w2) + Jl2[3 + rr] * (-i2d * e2[1] * w2));
#pragma unroll
          for (int cc = rr; cc < 3; ++cc) {
            const double h = (Jl1[rr] * wo1 * Jl1[cc] + Jl1[3 + rr] * wo1 * Jl1[3 + cc]) + (Jl2[rr] * wo2 * Jl2[cc] + Jl2[3 + rr] * wo2 * Jl2[3 + cc]);
            r[IM_HLL + u++] = h;
            if (cc == rr) md = fmax(md, fabs(h));
          }
        }
        u = 0;
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) {
          hpp[21 + rr] += Jp[rr] * (-i2d * e2[0] * w2) + Jp[6 + rr] * (-i2d * e2[1] * w2);
#pragma unroll
          for (int cc = rr; cc < 6; ++cc) hpp[u++] += Jp[rr] * wo2 * Jp[cc] + Jp[6 + rr] * wo2 * Jp[6 + cc];
#pragma unroll
          for (int cc = 0; cc < 3; ++cc) r[IM_HPL + rr * 3 + cc] = Jp[rr] * wo2 * Jl2[cc] + Jp[6 + rr] * wo2 * Jl2[3 + cc];
        }
      }
      im_reduce<IM_NR>(hpp, sh, lane, wv);
      if (iter == 0) {   // computeLambdaInit: the largest diagonal entry of every active vertex, landmarks included
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) md = fmax(md, __shfl_xor(md, off, 64));
        __syncthreads();
        if (lane == 0) sh.part[wv][IM_NR] = md;
        __syncthreads();
        md = fmax(fmax(sh.part[0][IM_NR], sh.part[1][IM_NR]), fmax(sh.part[2][IM_NR], sh.part[3][IM_NR]));
        md = fmax(md, fmax(fmax(fabs(hpp[0]), fabs(hpp[6])), fmax(fabs(hpp[11]), fabs(hpp[15]))));
        md = fmax(md, fmax(fabs(hpp[18]), fabs(hpp[20])));
        lm_begin(c, 0.0, md);
      }
      bool again = true;
      while (again) {   // at most ten trials: lm_trial counts them
        const double lambda = c.lambda;
        // ---- BlockSolver::solve with lambda on every diagonal: the Schur complement over the points (block_solver.hpp:354-480)
        double sc[IM_NR];
#pragma unroll
        for (int k = 0; k < IM_NR; ++k) sc[k] = 0.0;
        for (int q = tid; q < n; q += IM_T) {
          const double* r = rec + (size_t)q * IM_RS;
          double Di[9], BD[18];
          im_inv3_sym(r + IM_HLL, lambda, Di);
#pragma unroll
          for (int rr = 0; rr < 6; ++rr)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc)
              BD[rr * 3 + cc] = r[IM_HPL + rr * 3] * Di[cc] + r[IM_HPL + rr * 3 + 1] * Di[3 + cc] + r[IM_HPL + rr * 3 + 2] * Di[6 + cc];
          int u = 0;
#pragma unroll
          for (int rr = 0; rr < 6; ++rr) {
            sc[21 + rr] += BD[rr * 3] * r[IM_BL] + BD[rr * 3 + 1] * r[IM_BL + 1] + BD[rr * 3 + 2] * r[IM_BL + 2];
#pragma unroll
            for (int cc = rr; cc < 6; ++cc)
              sc[u++] += BD[rr * 3] * r[IM_HPL + cc * 3] + BD[rr * 3 + 1] * r[IM_HPL + cc * 3 + 1] + BD[rr * 3 + 2] * r[IM_HPL + cc * 3 + 2];
          }
        }
        im_reduce<IM_NR>(sc, sh, lane, wv);
        double xp[6];
        {
          int u = 0;
#pragma unroll
          for (int rr = 0; rr < 6; ++rr)
#pragma unroll
            for (int cc = rr; cc < 6; ++cc) { sc[u] = hpp[u] + (cc == rr ? lambda : 0.0) - sc[u]; ++u; }
#pragma unroll
          for (int rr = 0; rr < 6; ++rr) sc[21 + rr] = hpp[21 + rr] - sc[21 + rr];
        }
        const bool ok2 = im_solve6(sc, sc + 21, xp);
        if (!ok2) {
#pragma unroll
          for (int k = 0; k < 6; ++k) xp[k] = 0.0;
        }
        // ---- push, back-substitution xl = Dinv (bl - Hpl^T xp), oplus, the trial state's chi2 and computeScale's sum, one pass
        Tbk = T;
        T = se3_mul(se3_exp(xp), T);
        double tg[2] = {0.0, 0.0};
        for (int q = tid; q < n; q += IM_T) {
          double* r = rec + (size_t)q * IM_RS;
          double Di[9], cl[3], dx[3];
          im_inv3_sym(r + IM_HLL, lambda, Di);
#pragma unroll
          for (int cc = 0; cc < 3; ++cc) {
            double s = r[IM_BL + cc];
#pragma unroll
            for (int rr = 0; rr < 6; ++rr) s -= r[IM_HPL + rr * 3 + cc] * xp[rr];
            cl[cc] = s;
          }
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            dx[k] = ok2 ? Di[k * 3] * cl[0] + Di[k * 3 + 1] * cl[1] + Di[k * 3 + 2] * cl[2] : 0.0;
            r[IM_XBK + k] = r[IM_X + k];
            r[IM_X + k] += dx[k];
            tg[1] += dx[k] * (lambda * dx[k] + r[IM_BL + k]);
          }
          tg[0] += im_point_chi2<KB8>(cam, robust, delta, reinterpret_cast<const float*>(r + IM_WORDS), r + IM_X, T);
        }
        im_reduce<2>(tg, sh, lane, wv);
        double gain = tg[1];
#pragma unroll
        for (int k = 0; k < 6; ++k) gain += xp[k] * (lambda * xp[k] + hpp[21 + k]);
        const bool keep = lm_trial(c, tg[0], ok2, gain, &again);
        if (!keep) {   // pop
          T = Tbk;
          for (int q = tid; q < n; q += IM_T) {
            double* r = rec + (size_t)q * IM_RS;
#pragma unroll
            for (int k = 0; k < 3; ++k) r[IM_X + k] = r[IM_XBK + k];
          }
        }
        ++trials;
        if (again && stop_set()) { stopSeen = 1; again = false; }
      }
      if (lm_iteration_done(c)) break;
    }
    if (its > 0) chiLast = c.currentChi;
  }

  // ---- write-back (Optimizer.cc:276-361 with nLoopKF == 0): SetPose, SetWorldPos(estimate.cast<float>()); the depths of keyframe 1
  float Tf[12];
  im_pose_to_float(T, Tf);
  for (int q = tid; q < n; q += IM_T) {
    double* r = rec + (size_t)q * IM_RS;
    const float Xf[3] = {(float)r[IM_X], (float)r[IM_X + 1], (float)r[IM_X + 2]};
    r[IM_X] = (double)Xf[0]; r[IM_X + 1] = (double)Xf[1]; r[IM_X + 2] = (double)Xf[2];
    r[IM_BL] = (double)morbim::im_depth_key(morbim::im_kf1_depth(Xf));
  }
  __syncthreads();
  // ---- ComputeSceneMedianDepth(2): the key of rank (n - 1) / 2, fixed bit by bit from the top (integer counts: any order gives the same)
  float median = -1.f;
  if (n > 0) {
    uint32_t prefix = 0, mask = 0;
    int rank = morbim::im_median_rank(n);
    for (int bit = 31; bit >= 0; --bit) {
      int cnt = 0;
      for (int q = tid; q < n; q += IM_T) {
        const uint32_t key = (uint32_t)rec[(size_t)q * IM_RS + IM_BL];
        cnt += ((key & mask) == prefix && !((key >> bit) & 1u)) ? 1 : 0;
      }
      cnt = morbwave::sum_i32(cnt);
      __syncthreads();
      if (lane == 0) sh.ipart[wv] = cnt;
      __syncthreads();
      cnt = sh.ipart[0] + sh.ipart[1] + sh.ipart[2] + sh.ipart[3];
      if (rank >= cnt) { rank -= cnt; prefix |= 1u << bit; }
      mask |= 1u << bit;
    }
    median = morbim::im_key_depth(prefix);
  }
  const int status = morbim::im_status(median, n, a.minTracked);
  const float invMedianDepth = a.depthScale / median;
  const bool scale = status == morbim::IM_OK && a.depthScale != 0.f;
  if (scale) morbim::im_scale3(Tf + 9, invMedianDepth);   // Tc2w.translation() *= invMedianDepth
  float Ow2[3];
  morbim::im_camera_centre(Tf, Ow2);
  const float lastScale = a.P.scaleFactors[(a.P.nlevels - 1) & 15];
  for (int q = tid; q < n; q += IM_T) {
    const double* r = rec + (size_t)q * IM_RS;
    const int* wi = reinterpret_cast<const int*>(r + IM_WORDS);
    const int i = wi[6];
    float X[3] = {(float)r[IM_X], (float)r[IM_X + 1], (float)r[IM_X + 2]}, nrm[3], d2[2];
    if (scale) morbim::im_scale3(X, invMedianDepth);          // pMP->SetWorldPos(pMP->GetWorldPos() * invMedianDepth)
    morbim::im_point_fields(X, Ow2, a.P.scaleFactors[kp2[wi[7]].octave & 15], lastScale, nrm, d2);
    for (int k = 0; k < 3; ++k) { mpPos[3 * i + k] = X[k]; mpNormal[3 * i + k] = nrm[k]; }
    mpDist[2 * i] = d2[0]; mpDist[2 * i + 1] = d2[1];
    hasMP[i] = 1;
  }
  if (tid == 0) {
    for (int k = 0; k < 12; ++k) a.Tcw2[12 * p + k] = Tf[k];
    a.status[p] = status;
    a.stats[4 * p + morbim::IM_S_POINTS] = n; a.stats[4 * p + morbim::IM_S_ITERATIONS] = its;
    a.stats[4 * p + morbim::IM_S_TRIALS] = trials; a.stats[4 * p + morbim::IM_S_STOP_SEEN] = stopSeen;
    a.chi2[2 * p] = chiFirst; a.chi2[2 * p + 1] = chiLast;
    a.median[p] = median;
  }
}

template <bool KB8>
int im_launch(morb_optimizer* o, const ImArgs& a0, int nprob, hipStream_t st) {
  ImArgs a = a0;
  if (a.cap > IM_LDS_N) {
    { const int rc = grow(o->initialMap, (size_t)nprob * a.cap * IM_RS, &a.ws); if (rc != MORB_OK) return rc; }
    hipLaunchKernelGGL((k_initial_map<KB8, true>), dim3(nprob), dim3(IM_T), 0, st, a);
  } else {
    const size_t lds = (size_t)a.cap * IM_RS * sizeof(double);
    MORB_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_initial_map<KB8, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_initial_map<KB8, false>), dim3(nprob), dim3(IM_T), lds, st, a);
  }
  MORB_HIP_CHECK(hipGetLastError());
  return MORB_OK;
}

}  // namespace

extern "C" int morb_create_initial_map_monocular_batch(morb_optimizer* o, const morb_frame_params* P, const float* cam8, int kb8, int nprob, int cap,
                                                       const int* d_img1, const int* d_img2, const int* d_count, const morb_keypoint* d_kpsUn,
                                                       const int* d_matches12, const int* d_ok, const float* d_T21, const float* d_P3D,
                                                       const uint8_t* d_triangulated, int nIterations, int robust, float depthScale, int minTracked,
                                                       const unsigned char* d_stop, int* d_status, float* d_Tcw2, float* d_mpPos, float* d_mpNormal,
                                                       float* d_mpDist, uint8_t* d_hasMP, int* d_stats, double* d_chi2, float* d_median,
                                                       void* stream) {
  MORB_REQUIRE(o && P && d_img1 && d_img2 && d_count && d_kpsUn && d_matches12 && d_ok && d_T21 && d_P3D && d_triangulated, MORB_ERR_INVALID,
               "NULL argument");
  MORB_REQUIRE(d_status && d_Tcw2 && d_mpPos && d_mpNormal && d_mpDist && d_hasMP && d_stats && d_chi2 && d_median, MORB_ERR_INVALID, "NULL output");
  MORB_REQUIRE(kb8 == 0 || cam8, MORB_ERR_INVALID, "a KannalaBrandt8 camera needs cam8");
  MORB_REQUIRE(cap >= 1 && nIterations >= 0 && nprob >= 0, MORB_ERR_INVALID, "bad sizes");
  if (nprob == 0) return MORB_OK;
  MORB_ENTER(st, o, stream);
  ImArgs a;
  a.P = *P;
  if (cam8) for (int k = 0; k < 8; ++k) a.cam[k] = cam8[k];
  else { a.cam[0] = P->fx; a.cam[1] = P->fy; a.cam[2] = P->cx; a.cam[3] = P->cy; a.cam[4] = a.cam[5] = a.cam[6] = a.cam[7] = 0.f; }
  a.cap = cap; a.img1 = d_img1; a.img2 = d_img2; a.count = d_count; a.kps = d_kpsUn; a.matches12 = d_matches12; a.ok = d_ok; a.T21 = d_T21;
  a.P3D = d_P3D; a.triangulated = d_triangulated; a.nIterations = nIterations; a.robust = robust; a.depthScale = depthScale;
  a.minTracked = minTracked; a.stop = d_stop; a.status = d_status; a.Tcw2 = d_Tcw2; a.mpPos = d_mpPos; a.mpNormal = d_mpNormal;
  a.mpDist = d_mpDist; a.hasMP = d_hasMP; a.stats = d_stats; a.chi2 = d_chi2; a.median = d_median; a.ws = nullptr;
  return kb8 ? im_launch<true>(o, a, nprob, st) : im_launch<false>(o, a, nprob, st);
}
