// Sim3Solver (reference src/Sim3Solver.cc) for MI355X (gfx950), batched: one 256-thread workgroup per problem (pKF1, pKF2,
// vpMatched12, vpKeyFrameMatchedMP).  Each call restates, operation for operation in float:
//   * the constructor (:34-120): the kept correspondences compacted in KF1 feature order (ransac_block.h), camera-frame points
//     Rcw * Xw + tcw, FromCameraToImage of the MAP POINTS with each side's camera (Pinhole / KannalaBrandt8 project(Vector3f):
//     project of morb/camera_math.h, with glibc's atan2f / sinf / cosf), the truncated size_t thresholds 9.210 * sigma2;
//   * SetRansacParameters (:122-146) from the device-side N (include/morb/sim3_solver_math.h, ransac_math.h);
//   * iterate (:148-278) from state.iterations on: DUtils::Random::RandomInt + swap-with-back sampling on the caller's rand()
//     values (three per iteration, indexed by the global iteration number), ComputeSim3 (:285-392), CheckInliers (:394-414),
//     the running best with >= and the return at the first iteration with more than minInliers inliers.
// Mapping: the correspondences (points, projections, thresholds: 13 words each) live in LDS up to SS_LDS_N, in a global
// workspace beyond.  Hypotheses are built SS_B at a time, one lane each (Horn's closed form with an FP64 cyclic Jacobi
// for the 4 x 4 eigenproblem); their inliers are counted in iteration order, one wave per hypothesis
// (ballots), four at a time, and after every four the counts are scanned with the reference's rule, so the solver stops
// at the first success and no later hypothesis is ever reported.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "handles.h"
#include "morb/camera_math.h"
#include "libm_f32.h"
#include "morb_hip.h"
#include "morb/sim3_solver_math.h"
#include "ransac_block.h"

#ifndef MORB_SIM3_SOLVER_BATCH
#define MORB_SIM3_SOLVER_BATCH 64
#endif

namespace {

constexpr int SS_NT = 256;
constexpr int SS_NW = SS_NT / 64;
constexpr int SS_B = MORB_SIM3_SOLVER_BATCH;   // hypotheses built per batch (chosen by measurement)
constexpr int SS_LDS_N = 1024;                 // correspondences held in LDS; beyond, the global workspace
constexpr int SS_W = 13;                       // words per correspondence
constexpr int SS_HW = 40;                      // floats per hypothesis: T12 [12] (sR row-major, t), T21 [12], R [9], t [3], s
static_assert(SS_B % SS_NW == 0 && SS_B <= SS_NT, "batch");

using morbcam::Camera;
using namespace morbransac;

// R * x + t, R row-major: Eigen's 3-term sums taken left to right
__device__ __forceinline__ void affine(const float* R, const float* t, const float* x, float* o) {
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = R[r * 3] * x[0] + R[r * 3 + 1] * x[1] + R[r * 3 + 2] * x[2] + t[r];
}

// One cyclic-Jacobi rotation annihilating a[P][Q] (A <- J^T A J, V <- V J); constant indices, so nothing goes to scratch.
template <int P, int Q>
__device__ __forceinline__ void jrot(double (&a)[4][4], double (&v)[4][4]) {
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double akp = a[k][P], akq = a[k][Q];
    a[k][P] = c * akp - s * akq;
    a[k][Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double apk = a[P][k], aqk = a[Q][k];
    a[P][k] = c * apk - s * aqk;
    a[Q][k] = s * apk + c * aqk;
  }
  a[P][Q] = 0.0;
  a[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double vkp = v[k][P], vkq = v[k][Q];
    v[k][P] = c * vkp - s * vkq;
    v[k][Q] = s * vkp + c * vkq;
  }
}

// Sim3Solver::ComputeSim3 (:285-392) on the columns P1 / P2 (P[r][c]: coordinate r of point c); writes one hypothesis record.
__device__ __forceinline__ void compute_sim3(const float (&P1)[3][3], const float (&P2)[3][3], bool fixScale, float* h) {
  float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {   // ComputeCentroid: rowwise().sum() / cols()
    O1[r] = (P1[r][0] + P1[r][1] + P1[r][2]) / 3.0f;
    O2[r] = (P2[r][0] + P2[r][1] + P2[r][2]) / 3.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) { Pr1[r][c] = P1[r][c] - O1[r]; Pr2[r][c] = P2[r][c] - O2[r]; }
  }
  float M[3][3];   // Pr2 * Pr1^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[i][j] = Pr2[i][0] * Pr1[j][0] + Pr2[i][1] * Pr1[j][1] + Pr2[i][2] * Pr1[j][2];
  // the N entries: float sums of float entries, held in a double, stored in a Matrix4f
  const float N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0];
  const float N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2];
  const float N33 = -M[0][0] + M[1][1] - M[2][2], N34 = M[1][2] + M[2][1], N44 = -M[0][0] - M[1][1] + M[2][2];
  double a[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}};
  double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  double fro2 = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) fro2 += a[i][j] * a[i][j];
  for (int sweep = 0; sweep < 16; ++sweep) {
    const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[0][3] * a[0][3] + a[1][2] * a[1][2] + a[1][3] * a[1][3] + a[2][3] * a[2][3];
    if (off <= 1e-30 * fro2) break;
    jrot<0, 1>(a, v); jrot<0, 2>(a, v); jrot<0, 3>(a, v); jrot<1, 2>(a, v); jrot<1, 3>(a, v); jrot<2, 3>(a, v);
  }
  // eval.maxCoeff(&maxIndex) over the float eigenvalues: the first maximum
  int maxIndex = 0;
  float best = (float)a[0][0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if ((float)a[k][k] > best) { best = (float)a[k][k]; maxIndex = k; }
  double e[4] = {v[0][0], v[1][0], v[2][0], v[3][0]};
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (maxIndex == k) { e[0] = v[0][k]; e[1] = v[1][k]; e[2] = v[2][k]; e[3] = v[3][k]; }
  const double en = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3]);
  const float q0 = (float)(e[0] / en);
  float vec[3] = {(float)(e[1] / en), (float)(e[2] / en), (float)(e[3] / en)};
  const float vn = sqrtf(vec[0] * vec[0] + vec[1] * vec[1] + vec[2] * vec[2]);
  const double ang = morbs3::sim3s_atan2((double)vn, (double)q0);
  const float f = (float)(2 * ang);   // 2 * ang * vec / vec.norm(): the double factor becomes the float scalar of the expression
#pragma unroll
  for (int k = 0; k < 3; ++k) vec[k] = f * vec[k] / vn;
  // Sophus::SO3f::exp (so3.hpp:583-619), then Quaternion::toRotationMatrix
  const float theta_sq = vec[0] * vec[0] + vec[1] * vec[1] + vec[2] * vec[2];
  float imag, real;
  if (theta_sq < 1e-5f * 1e-5f) {
    const float theta_po4 = theta_sq * theta_sq;
    imag = 0.5f - (float)(1.0 / 48.0) * theta_sq + (float)(1.0 / 3840.0) * theta_po4;
    real = 1.0f - (float)(1.0 / 8.0) * theta_sq + (float)(1.0 / 384.0) * theta_po4;
  } else {
    const float theta = sqrtf(theta_sq);
    const float half = 0.5f * theta;
    imag = morbm::sinf_glibc(half) / theta;
    real = morbm::cosf_glibc(half);
  }
  const float qw = real, qx = imag * vec[0], qy = imag * vec[1], qz = imag * vec[2];
  const float tx = 2.0f * qx, ty = 2.0f * qy, tz = 2.0f * qz;
  const float twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy,
              tzz = tz * qz;
  const float R[3][3] = {{1.0f - (tyy + tzz), txy - twz, txz + twy},
                         {txy + twz, 1.0f - (txx + tzz), tyz - twx},
                         {txz - twy, tyz + twx, 1.0f - (txx + tyy)}};
  float s = 1.0f;
  if (!fixScale) {
    float P3[3][3];   // mR12i * Pr2
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) P3[i][c] = R[i][0] * Pr2[0][c] + R[i][1] * Pr2[1][c] + R[i][2] * Pr2[2][c];
    // (Pr1.array() * P3.array()).sum() and (P3.array() * P3.array()).sum(): float sums in storage (column-major) order
    float nom = Pr1[0][0] * P3[0][0], den = P3[0][0] * P3[0][0];
#pragma unroll
    for (int k = 1; k < 9; ++k) {
      const int r = k % 3, c = k / 3;
      nom += Pr1[r][c] * P3[r][c];
      den += P3[r][c] * P3[r][c];
    }
    s = (float)((double)nom / (double)den);
  }
  float sR[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) sR[i] = s * R[i / 3][i % 3];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = O1[i] - (sR[i * 3] * O2[0] + sR[i * 3 + 1] * O2[1] + sR[i * 3 + 2] * O2[2]);
  const float inv = (float)(1.0 / (double)s);   // (1.0 / ms12i) * R^T: the double factor becomes a float scalar
  float sRi[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) sRi[i * 3 + j] = inv * R[j][i];
#pragma unroll
  for (int i = 0; i < 9; ++i) { h[i] = sR[i]; h[12 + i] = sRi[i]; h[24 + i] = R[i / 3][i % 3]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    h[9 + i] = t[i];
    h[21 + i] = -(sRi[i * 3] * t[0] + sRi[i * 3 + 1] * t[1] + sRi[i * 3 + 2] * t[2]);
    h[33 + i] = t[i];
  }
  h[36] = s;
}

struct Corr {   // structure of arrays, `stride` entries each
  float *x1, *x2, *p1, *p2, *e1, *e2;
  int* id;
  int stride;
};
__device__ inline Corr ss_carve(float* base, int stride) {
  Corr c;
  c.x1 = base; c.x2 = base + 3 * stride; c.p1 = base + 6 * stride; c.p2 = base + 8 * stride;
  c.e1 = base + 10 * stride; c.e2 = base + 11 * stride; c.id = (int*)(base + 12 * stride);
  c.stride = stride;
  return c;
}

// CheckInliers' test of correspondence i against hypothesis h (:394-414)
__device__ __forceinline__ bool is_inlier(const Corr& C, int i, const float* T12, const float* T21, const Camera& c1, const Camera& c2) {
  const int S = C.stride;
  const float X2[3] = {C.x2[i], C.x2[S + i], C.x2[2 * S + i]};
  float P[3], uv[2];
  affine(T12, T12 + 9, X2, P);
  morbcam::project(c1, P, uv[0], uv[1]);
  const float d0 = C.p1[i] - uv[0], d1 = C.p1[S + i] - uv[1];
  const float err1 = d0 * d0 + d1 * d1;
  const float X1[3] = {C.x1[i], C.x1[S + i], C.x1[2 * S + i]};
  affine(T21, T21 + 9, X1, P);
  morbcam::project(c2, P, uv[0], uv[1]);
  const float f0 = uv[0] - C.p2[i], f1 = uv[1] - C.p2[S + i];
  const float err2 = f0 * f0 + f1 * f1;
  return err1 < C.e1[i] && err2 < C.e2[i];
}

struct SsShared {
  float corr[SS_LDS_N * SS_W];
  float hyp[SS_B][SS_HW];
  float best[SS_HW];
  int cnt[SS_B];
  int wcount[SS_NW];
  int N, nc, iters, bestInliers, improved, conv;
};

__device__ inline bool kept(uint8_t en) {   // matched, pMP1 present, neither bad, both keyframe indices >= 0
  return (en & 1) && (en & 2) && !(en & 4) && !(en & 8) && !(en & 16) && !(en & 32);
}

__device__ __forceinline__ void solve(SsShared& sh, const Corr& C, int p, int n, int cap, const morb_sim3_solver_params& prm, const Camera& c1, const Camera& c2,
                      const uint8_t* __restrict__ d_entry, const float* __restrict__ d_Xw1, const float* __restrict__ d_Xw2,
                      const float* __restrict__ d_s2_1, const float* __restrict__ d_s2_2, int nIterations, const int* __restrict__ d_rand,
                      int randCap, morb_sim3_solver_state* __restrict__ d_state, uint8_t* __restrict__ d_inliers, int* __restrict__ d_hyp,
                      int hypCap) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const size_t pc = (size_t)p * cap;
  const int S = C.stride;
  // ---- the constructor: compaction in feature order ----
  for (int base = 0; base < n; base += SS_NT) {
    const int i = base + t;
    const bool valid = i < n && kept(d_entry[pc + i]);
    const int c = ordered_slot(valid, lane, wv, sh.wcount, &sh.nc);
    if (valid) {
      float X1[3], X2[3], uv[2];
      affine(prm.T1w, prm.T1w + 9, d_Xw1 + (pc + i) * 3, X1);
      affine(prm.T2w, prm.T2w + 9, d_Xw2 + (pc + i) * 3, X2);
#pragma unroll
      for (int r = 0; r < 3; ++r) { C.x1[r * S + c] = X1[r]; C.x2[r * S + c] = X2[r]; }
      morbcam::project(c1, X1, uv[0], uv[1]);
      C.p1[c] = uv[0]; C.p1[S + c] = uv[1];
      morbcam::project(c2, X2, uv[0], uv[1]);
      C.p2[c] = uv[0]; C.p2[S + c] = uv[1];
      C.e1[c] = morbs3::sim3s_max_error(d_s2_1[pc + i]);
      C.e2[c] = morbs3::sim3s_max_error(d_s2_2[pc + i]);
      C.id[c] = i;
    }
    ordered_commit<SS_NW>(sh.wcount, &sh.nc);
  }
  const int N = sh.N;
  const int budget = morbs3::sim3s_budget(N, prm.minInliers, prm.probability, prm.maxIterations);
  const int it0 = d_state[p].iterations;
  if (t == 0) {
    sh.iters = it0;
    sh.bestInliers = d_state[p].bestInliers;
    sh.improved = 0;
    sh.conv = 0;
  }
  if (N < prm.minInliers || N < 3) {   // iterate's early return (N < 3 only with minInliers < 3: see include/morb_hip.h)
    if (t == 0) {
      morb_sim3_solver_state& st = d_state[p];
      st.N = N; st.budget = budget; st.converged = 0; st.noMore = 1; st.nInliers = 0; st.convergedAt = -1;
      identity16(st.sim3);
    }
    return;
  }
  int end = budget;
  if (nIterations < end - it0) end = it0 + (nIterations > 0 ? nIterations : 0);
  if (randCap / 3 < end) end = randCap / 3;
  __syncthreads();
  for (int b0 = it0; b0 < end; b0 += SS_B) {
    const int nb = min(SS_B, end - b0);
    if (t < nb) {   // one lane per hypothesis: sampling (RandomInt + swap with back) and ComputeSim3
      const int g = b0 + t;
      const int* r = d_rand + (size_t)p * randCap + 3 * (size_t)g;
      const int a1 = random_int(r[0], N);
      const int a2 = random_int(r[1], N - 1);
      const int a3 = random_int(r[2], N - 2);
      const int last1 = (a1 == N - 2) ? N - 1 : N - 2;   // vAvailableIndices[N - 2] after the first removal
      const int idx[3] = {a1, (a2 == a1) ? N - 1 : a2, (a3 == a2) ? last1 : ((a3 == a1) ? N - 1 : a3)};
      float P1[3][3], P2[3][3];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) { P1[rr][c] = C.x1[rr * S + idx[c]]; P2[rr][c] = C.x2[rr * S + idx[c]]; }
      compute_sim3(P1, P2, prm.fixScale != 0, sh.hyp[t]);
    }
    __syncthreads();
    for (int h0 = 0; h0 < nb; h0 += SS_NW) {   // CheckInliers in iteration order, one wave per hypothesis
      const int h = h0 + wv;
      if (h < nb) {
        float T12[12], T21[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) { T12[k] = sh.hyp[h][k]; T21[k] = sh.hyp[h][12 + k]; }
        int cnt = 0;
        for (int base = 0; base < N; base += 64) {
          const int i = base + lane;
          const bool in = i < N && is_inlier(C, i, T12, T21, c1, c2);
          cnt += __popcll(__ballot(in));
        }
        if (lane == 0) sh.cnt[h] = cnt;
      }
      __syncthreads();
      if (t == 0) {   // the bookkeeping of iterate, in iteration order
        const int hend = min(h0 + SS_NW, nb);
        for (int hh = h0; hh < hend; ++hh) {
          const int g = b0 + hh, c = sh.cnt[hh];
          sh.iters = g + 1;
          if (d_hyp && g < hypCap) d_hyp[(size_t)p * hypCap + g] = c;
          if (c >= sh.bestInliers) {
            sh.bestInliers = c;
            sh.improved = 1;
            for (int k = 0; k < 37; ++k) sh.best[k] = sh.hyp[hh][k];
            if (c > prm.minInliers) { sh.conv = 1; break; }
          }
        }
      }
      __syncthreads();
      if (sh.conv) break;
    }
    if (sh.conv) break;
  }
  const bool conv = sh.conv != 0;
  if (conv) {   // the inlier mask of the converged hypothesis, by KF1 feature
    float T12[12], T21[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { T12[k] = sh.best[k]; T21[k] = sh.best[12 + k]; }
    for (int i = t; i < N; i += SS_NT)
      if (is_inlier(C, i, T12, T21, c1, c2)) d_inliers[pc + C.id[i]] = 1;
  }
  if (t == 0) {
    morb_sim3_solver_state& st = d_state[p];
    st.N = N;
    st.budget = budget;
    st.iterations = sh.iters;
    st.bestInliers = sh.bestInliers;
    st.converged = conv;
    st.noMore = !conv && sh.iters >= budget;
    st.nInliers = conv ? sh.bestInliers : 0;
    st.convergedAt = conv ? sh.iters - 1 : -1;
    if (sh.improved) {
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) st.bestT12[r * 4 + c] = sh.best[r * 3 + c];
        st.bestT12[r * 4 + 3] = sh.best[9 + r];
      }
      st.bestT12[12] = 0.f; st.bestT12[13] = 0.f; st.bestT12[14] = 0.f; st.bestT12[15] = 1.f;
      for (int k = 0; k < 9; ++k) st.bestR[k] = sh.best[24 + k];
      for (int k = 0; k < 3; ++k) st.bestt[k] = sh.best[33 + k];
      st.bestScale = sh.best[36];
    }
    for (int k = 0; k < 16; ++k) st.sim3[k] = sh.improved ? st.bestT12[k] : ((k % 5 == 0) ? 1.f : 0.f);
  }
}

__global__ __launch_bounds__(SS_NT) void k_sim3_solver(int cap, const morb_sim3_solver_params* __restrict__ d_params,
                                                       const uint8_t* __restrict__ d_entry, const float* __restrict__ d_Xw1,
                                                       const float* __restrict__ d_Xw2, const float* __restrict__ d_s2_1,
                                                       const float* __restrict__ d_s2_2, int nIterations, const int* __restrict__ d_rand,
                                                       int randCap, morb_sim3_solver_state* __restrict__ d_state,
                                                       uint8_t* __restrict__ d_inliers, int* __restrict__ d_hyp, int hypCap,
                                                       char* __restrict__ ws, size_t wsPitch) {
  __shared__ SsShared sh;
  const int p = blockIdx.x, t = threadIdx.x;
  const morb_sim3_solver_params prm = d_params[p];
  const int n = min(max(prm.n, 0), cap);
  const size_t pc = (size_t)p * cap;
  Camera c1, c2;
  c1.kb8 = prm.cam1[0] != 0.f; c2.kb8 = prm.cam2[0] != 0.f;
  for (int i = 0; i < 8; ++i) { c1.p[i] = prm.cam1[1 + i]; c2.p[i] = prm.cam2[1 + i]; }
  // vbInliers = vector<bool>(mN1, false), and N
  for (int i = t; i < cap; i += SS_NT) d_inliers[pc + i] = 0;
  if (t == 0) { sh.N = 0; sh.nc = 0; }
  __syncthreads();
  block_count<SS_NT>(n, &sh.N, [=](int i) { return kept(d_entry[pc + i]); });
  // two inlined call sites: in the first the correspondence arrays are known to be LDS, so it addresses them with ds_* instructions
  if (sh.N <= SS_LDS_N)
    solve(sh, ss_carve(sh.corr, SS_LDS_N), p, n, cap, prm, c1, c2, d_entry, d_Xw1, d_Xw2, d_s2_1, d_s2_2, nIterations, d_rand, randCap,
                d_state, d_inliers, d_hyp, hypCap);
  else
    solve(sh, ss_carve((float*)(ws + (size_t)p * wsPitch), cap), p, n, cap, prm, c1, c2, d_entry, d_Xw1, d_Xw2, d_s2_1, d_s2_2,
                 nIterations, d_rand, randCap, d_state, d_inliers, d_hyp, hypCap);
}

}  // namespace

extern "C" int morb_sim3_solver_batch(morb_optimizer* o, int nprob, int cap, const morb_sim3_solver_params* d_params, const uint8_t* d_entry,
                                      const float* d_Xw1, const float* d_Xw2, const float* d_sigma2_1, const float* d_sigma2_2,
                                      int nIterations, const int* d_rand, int randCap, morb_sim3_solver_state* d_state,
                                      uint8_t* d_inliers, int* d_hypInliers, int hypCap, void* stream) {
  MORB_REQUIRE(o && d_params && d_entry && d_Xw1 && d_Xw2 && d_sigma2_1 && d_sigma2_2 && d_state && d_inliers, MORB_ERR_INVALID,
               "NULL argument");
  MORB_REQUIRE(nprob > 0 && cap > 0 && randCap >= 0 && (d_rand || randCap == 0) && (d_hypInliers == nullptr || hypCap >= 0),
               MORB_ERR_INVALID, "bad sizes");
  MORB_ENTER(st, o, stream);
  size_t pitch;
  char* ws;
  const int rc = morb::grow_beyond_lds(o->spill, nprob, cap, SS_LDS_N, SS_W, &ws, &pitch);
  if (rc != MORB_OK) return rc;
  hipLaunchKernelGGL(k_sim3_solver, dim3(nprob), dim3(SS_NT), 0, st, cap, d_params, d_entry, d_Xw1, d_Xw2, d_sigma2_1, d_sigma2_2,
                     nIterations, d_rand, randCap, d_state, d_inliers, d_hypInliers, hypCap, ws, pitch);
  MORB_HIP_CHECK(hipGetLastError());
  return MORB_OK;
}
