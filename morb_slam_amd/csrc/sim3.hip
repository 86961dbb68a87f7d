// Optimizer::OptimizeSim3 (reference src/Optimizer.cc:2065-2322) for MI355X (gfx950), batched: one 256-thread workgroup per
// problem (pKF1, pKF2, vpMatches1, g2oS12).  Each workgroup runs the reference's whole procedure:
//   * the edge set (:2118-2231): per KF1 feature i in ascending order, an EdgeSim3ProjectXYZ (e12) and an
//     EdgeInverseSim3ProjectXYZ (e21) per correspondence, camera-frame points in float, Huber delta sqrtf(th2);
//   * g2o's OptimizationAlgorithmLevenberg (optimization_algorithm_levenberg.cpp:61-169) over one VertexSim3Expmap
//     (OptimizableTypes.h:166-187), the 7x7 system solved by Eigen::LDLT's pivoted algorithm (LinearSolverDense);
//   * numeric Jacobians as BaseBinaryEdge::linearizeOplus takes them (base_binary_edge.hpp:130-205: central differences,
//     delta = 1e-9, 14 computeError calls per edge), with the whole error chain restated operation for operation in FP64:
//     the Sim3 exponential with its eps = 1e-5 branches (types/sim3.h), Eigen's Quaterniond(Matrix3d), map / inverse,
//     Pinhole::project(Vector3d) and KannalaBrandt8::project(Vector3d) (float atan2f / sqrtf inside, glibc's bits via libm_f32.h; cos / sin
//     of the double psi via libm_f64.h);
//   * every sum over the edges (J^T W J, J^T W e, the robust chi2) in g2o's insertion order e12_0, e21_0, e12_1, ...: the per-edge
//     contributions go to a workspace, then 36 lanes each walk the edge list;
//   * the two phases (:2233-2320), including the stale errors of a failed last trial in the phase-1 inlier test.
// exp(+-1e-9) of the perturbed scale steps are glibc's values as constants (tests/test_sim3_cpu.py checks them against the
// host libm); sin / cos / exp everywhere else are glibc's (libm_f64.h, checked there against the host libm).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "common.h"
#include "handles.h"
#include "libm_f32.h"
#include "libm_f64.h"
#include "morb/camera_math.h"
#include "quat_huber.h"
#include "sim3_math.h"

namespace {

constexpr int S3_NT = 256;
constexpr int S3_NCON = 36;                     // 28 lower-triangle entries of H, 7 of b, the robust chi2
constexpr double S3_EXP_P = 0x1.000000044b830p+0;    // glibc exp(+1e-9)
constexpr double S3_EXP_M = 0x1.fffffff768fa1p-1;    // glibc exp(-1e-9)
constexpr int S3_CORR = 12;                     // doubles per correspondence: X2c[3] X1c[3] obs1[2] obs2[2] info1 info2

using morbcam::Camera;   // (the Sim3 algebra and the exponential: sim3_math.h)

// ---- cameras (Pinhole.cpp:38-44, KannalaBrandt8.cpp:48-64) ----------------------------------------------------
__device__ __forceinline__ void cam_project(const Camera& c, const double* v, double* uv) {
  if (!c.kb8) {
    uv[0] = (double)c.p[0] * v[0] / v[2] + (double)c.p[2];
    uv[1] = (double)c.p[1] * v[1] / v[2] + (double)c.p[3];
    return;
  }
  const double x2_plus_y2 = v[0] * v[0] + v[1] * v[1];
  const double theta = morbm::atan2f_glibc(sqrtf((float)x2_plus_y2), (float)v[2]);
  const double psi = morbm::atan2f_glibc((float)v[1], (float)v[0]);
  const double theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta3 * theta2, theta7 = theta5 * theta2,
               theta9 = theta7 * theta2;
  const double r = theta + (double)c.p[4] * theta3 + (double)c.p[5] * theta5 + (double)c.p[6] * theta7 + (double)c.p[7] * theta9;
  double sp, cp;   // cos(psi) and sin(psi) of one function: one sincos call in a compiled reference
  morbm64::sincos_glibc(psi, &sp, &cp);
  uv[0] = (double)c.p[0] * r * cp + (double)c.p[2];
  uv[1] = (double)c.p[1] * r * sp + (double)c.p[3];
}

// error of edge `dir` (0: e12 = obs1 - cam1(S.map(X2c)), 1: e21 = obs2 - cam2(S^-1.map(X1c))) of correspondence `cr`
__device__ __forceinline__ void edge_error(const Sim3d& S, int dir, const double* cr, const Camera& c1, const Camera& c2, double* e) {
  double x[3], uv[2];
  if (dir == 0) {
    sim3_map(S, cr, x);
    cam_project(c1, x, uv);
    e[0] = cr[6] - uv[0]; e[1] = cr[7] - uv[1];
  } else {
    sim3_map(sim3_inverse(S), cr + 3, x);
    cam_project(c2, x, uv);
    e[0] = cr[8] - uv[0]; e[1] = cr[9] - uv[1];
  }
}
__device__ __forceinline__ double chi2_of(const double* e, double info) { return e[0] * (info * e[0]) + e[1] * (info * e[1]); }
// the perturbed estimate Sim3(+-delta e_d) * S of linearizeOplus (VertexSim3Expmap::oplusImpl: update[6] = 0 with a fixed scale)
__device__ __forceinline__ Sim3d perturbed(const Sim3d& S, int d, bool plus, bool fixScale) {
  double u[7] = {0, 0, 0, 0, 0, 0, 0};
  u[d] = plus ? S3_DELTA : -S3_DELTA;
  if (fixScale) u[6] = 0;
  const double s = u[6] == 0 ? 1.0 : (plus ? S3_EXP_P : S3_EXP_M);
  return sim3_mul(sim3_exp(u, s), S);
}

// Eigen::LDLT<MatrixXd> (LDLT.h: ldlt_inplace<Lower>::unblocked, diagonal pivoting; solve with the min() cutoff on D);
// returns isPositive().  H is 7x7 row-major, only its lower triangle is read.
__device__ bool ldlt7_solve(const double* Hin, const double* b, double* x) {
  double m[49];
  for (int i = 0; i < 49; ++i) m[i] = Hin[i];
  int tr[7];
  double temp[7];
  int sign = 0;   // 0 ZeroSign, 1 PositiveSemiDef, 2 NegativeSemiDef, 3 Indefinite
  for (int k = 0; k < 7; ++k) {
    int big = k;
    double bigv = fabs(m[k * 8]);
    for (int i = k + 1; i < 7; ++i)
      if (fabs(m[i * 8]) > bigv) { bigv = fabs(m[i * 8]); big = i; }
    tr[k] = big;
    if (k != big) {
      for (int j = 0; j < k; ++j) { const double t = m[k * 7 + j]; m[k * 7 + j] = m[big * 7 + j]; m[big * 7 + j] = t; }
      for (int i = big + 1; i < 7; ++i) { const double t = m[i * 7 + k]; m[i * 7 + k] = m[i * 7 + big]; m[i * 7 + big] = t; }
      { const double t = m[k * 8]; m[k * 8] = m[big * 8]; m[big * 8] = t; }
      for (int i = k + 1; i < big; ++i) { const double t = m[i * 7 + k]; m[i * 7 + k] = m[big * 7 + i]; m[big * 7 + i] = t; }
    }
    if (k > 0) {
      for (int j = 0; j < k; ++j) temp[j] = m[j * 8] * m[k * 7 + j];
      double dot = 0;
      for (int j = 0; j < k; ++j) dot += m[k * 7 + j] * temp[j];
      m[k * 8] -= dot;
      for (int i = k + 1; i < 7; ++i)
        for (int j = 0; j < k; ++j) m[i * 7 + k] -= m[i * 7 + j] * temp[j];
    }
    const double akk = m[k * 8];
    const bool valid = fabs(akk) > 0;
    if (k == 0 && !valid) { sign = 0; for (int j = 0; j < 7; ++j) tr[j] = j; break; }
    if (valid)
      for (int i = k + 1; i < 7; ++i) m[i * 7 + k] /= akk;
    if (sign == 1) { if (akk < 0) sign = 3; }
    else if (sign == 2) { if (akk > 0) sign = 3; }
    else if (sign == 0) { if (akk > 0) sign = 1; else if (akk < 0) sign = 2; }
  }
  if (!(sign == 1 || sign == 0)) return false;
  double y[7];
  for (int i = 0; i < 7; ++i) y[i] = b[i];
  for (int k = 0; k < 7; ++k) { const double t = y[k]; y[k] = y[tr[k]]; y[tr[k]] = t; }
  for (int i = 0; i < 7; ++i)
    for (int j = 0; j < i; ++j) y[i] -= m[i * 7 + j] * y[j];
  for (int i = 0; i < 7; ++i) {
    if (fabs(m[i * 8]) > DBL_MIN) y[i] /= m[i * 8];
    else y[i] = 0;
  }
  for (int i = 6; i >= 0; --i)
    for (int j = i + 1; j < 7; ++j) y[i] -= m[j * 7 + i] * y[j];
  for (int k = 6; k >= 0; --k) { const double t = y[k]; y[k] = y[tr[k]]; y[tr[k]] = t; }
  for (int i = 0; i < 7; ++i) x[i] = y[i];
  return true;
}

struct S3Work {   // one problem's slice of the workspace
  double* corr;   // [cap][S3_CORR]
  int* idx;       // [cap] KF1 feature of correspondence c
  int* act;       // [cap] edges of c still in the graph
  double* chi;    // [2 cap] chi2 of the last computeError of each edge
  double* con;    // [S3_NCON][2 cap] per-edge contributions (edge order 2 c + dir)
};
__host__ __device__ inline size_t s3_bytes_per_problem(int cap) {
  auto al = [](size_t v) { return (v + 255) / 256 * 256; };
  return al((size_t)cap * S3_CORR * 8) + 2 * al((size_t)cap * 4) + al((size_t)cap * 16) + al((size_t)cap * 16 * S3_NCON);
}
__device__ inline S3Work s3_carve(char* base, int cap) {
  auto al = [](size_t v) { return (v + 255) / 256 * 256; };
  S3Work w;
  w.corr = (double*)base; base += al((size_t)cap * S3_CORR * 8);
  w.idx = (int*)base; base += al((size_t)cap * 4);
  w.act = (int*)base; base += al((size_t)cap * 4);
  w.chi = (double*)base; base += al((size_t)cap * 16);
  w.con = (double*)base;
  return w;
}

struct S3Shared {
  Sim3d S, T;                  // current estimate, trial estimate
  double sum[S3_NCON];
  double x[7];
  double lambda, currentChi, iniChi;
  int ni, nBad, qmax, ok2, cont, stop, nc, nBad1, nIn, iters, trials;
  int wcount[S3_NT / 64];
};

// errors (and, with build, linearizeOplus + constructQuadraticForm) of every active edge at S; edge order 2 c + dir
template <bool BUILD>
__device__ void eval_edges(const S3Work& w, int nc, int E2, const Sim3d& S, bool robust, double delta, bool fixScale, const Camera& c1,
                           const Camera& c2) {
  for (int e = threadIdx.x; e < 2 * nc; e += S3_NT) {
    const int c = e >> 1, dir = e & 1;
    if (!w.act[c]) continue;
    const double* cr = w.corr + (size_t)c * S3_CORR;
    const double info = cr[10 + dir];
    double err[2];
    edge_error(S, dir, cr, c1, c2, err);
    const double chi = chi2_of(err, info);
    double rho1 = 1.0;
    const double rho0 = robust ? huber(delta, chi, &rho1) : chi;
    w.chi[e] = chi;
    w.con[(size_t)35 * E2 + e] = rho0;
    if (!BUILD) continue;
    double J[2][7];
    const double scalar = 1.0 / (2 * S3_DELTA);
    for (int d = 0; d < 7; ++d) {
      double ep[2], em[2];
      edge_error(perturbed(S, d, true, fixScale), dir, cr, c1, c2, ep);
      edge_error(perturbed(S, d, false, fixScale), dir, cr, c1, c2, em);
      ep[0] -= em[0]; ep[1] -= em[1];
      J[0][d] = scalar * ep[0]; J[1][d] = scalar * ep[1];
    }
    const double wo = rho1 * info;
    double omr[2] = {-(info * err[0]), -(info * err[1])};
    if (robust) { omr[0] *= rho1; omr[1] *= rho1; }
    int k = 0;
    for (int r = 0; r < 7; ++r)
      for (int cc = 0; cc <= r; ++cc, ++k) w.con[(size_t)k * E2 + e] = (J[0][r] * wo) * J[0][cc] + (J[1][r] * wo) * J[1][cc];
    for (int r = 0; r < 7; ++r) w.con[(size_t)(28 + r) * E2 + e] = J[0][r] * omr[0] + J[1][r] * omr[1];
  }
}
// edge-order sum of contribution row k over the active edges (one lane)
__device__ double ordered_sum(const S3Work& w, int nc, int E2, int k) {
  double acc = 0;
  const double* row = w.con + (size_t)k * E2;
  for (int c = 0; c < nc; ++c) {
    if (!w.act[c]) continue;
    acc += row[2 * c];
    acc += row[2 * c + 1];
  }
  return acc;
}

// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg, after initializeOptimization (lambda restarts)
__device__ void lm_optimize(S3Shared& sh, const S3Work& w, int E2, int iterations, bool robust, double delta, bool fixScale, const Camera& c1,
                            const Camera& c2) {
  const int t = threadIdx.x;
  const int nc = sh.nc;
  if (t == 0) { sh.iters = 0; sh.trials = 0; for (int i = 0; i < 7; ++i) sh.x[i] = 0; }
  __syncthreads();
  for (int it = 0; it < iterations; ++it) {
    eval_edges<true>(w, nc, E2, sh.S, robust, delta, fixScale, c1, c2);
    __syncthreads();
    if (t < S3_NCON) sh.sum[t] = ordered_sum(w, nc, E2, t);
    __syncthreads();
    if (t == 0) {
      sh.currentChi = sh.sum[35];
      sh.iniChi = sh.currentChi;
      if (it == 0) {   // computeLambdaInit: tau * max |H_jj|, tau = 1e-5
        double maxDiagonal = 0.;
        for (int j = 0; j < 7; ++j) maxDiagonal = fmax(fabs(sh.sum[j * (j + 1) / 2 + j]), maxDiagonal);
        sh.lambda = 1e-5 * maxDiagonal;
        sh.ni = 2;
        sh.nBad = 0;
      }
      sh.qmax = 0;
    }
    __syncthreads();
    double rho = 0;   // meaningful on thread 0
    for (;;) {
      if (t == 0) {
        double H[49];
        for (int r = 0, k = 0; r < 7; ++r)
          for (int c = 0; c <= r; ++c, ++k) { H[r * 7 + c] = sh.sum[k]; H[c * 7 + r] = sh.sum[k]; }
        for (int j = 0; j < 7; ++j) H[j * 8] += sh.lambda;
        double xn[7];
        sh.ok2 = ldlt7_solve(H, sh.sum + 28, xn);
        if (sh.ok2)
          for (int j = 0; j < 7; ++j) sh.x[j] = xn[j];
        double u[7];
        for (int j = 0; j < 7; ++j) u[j] = sh.x[j];
        if (fixScale) u[6] = 0;
        // (|u[6]| >= 512 would overflow the scale anyway: there the device library's exp)
        sh.T = sim3_mul(sim3_exp(u, fabs(u[6]) < 512.0 ? morbm64::exp_glibc(u[6]) : exp(u[6])), sh.S);
      }
      __syncthreads();
      eval_edges<false>(w, nc, E2, sh.T, robust, delta, fixScale, c1, c2);
      __syncthreads();
      if (t == 0) {
        double tempChi = ordered_sum(w, nc, E2, 35);
        if (!sh.ok2) tempChi = DBL_MAX;
        rho = (sh.currentChi - tempChi);
        double scale = 0.;
        for (int j = 0; j < 7; ++j) scale += sh.x[j] * (sh.lambda * sh.x[j] + sh.sum[28 + j]);
        scale += 1e-3;
        rho /= scale;
        if (rho > 0 && isfinite(tempChi)) {
          const double q = 2 * rho - 1;
          double alpha = 1. - cube_rn(q);
          alpha = fmin(alpha, 2. / 3.);
          const double scaleFactor = fmax(1. / 3., alpha);
          sh.lambda *= scaleFactor;
          sh.ni = 2;
          sh.currentChi = tempChi;
          sh.S = sh.T;
        } else {
          sh.lambda *= sh.ni;
          sh.ni *= 2;
        }
        sh.qmax++;
        sh.trials++;
        sh.cont = (rho < 0 && sh.qmax < 10);
      }
      __syncthreads();
      if (!sh.cont) break;
      __syncthreads();
    }
    if (t == 0) {
      sh.iters++;
      sh.stop = 0;
      if (sh.qmax == 10 || rho == 0) sh.stop = 1;
      else {
        if ((sh.iniChi - sh.currentChi) * 1e3 < sh.iniChi) sh.nBad++;
        else sh.nBad = 0;
        if (sh.nBad >= 3) sh.stop = 1;
      }
    }
    __syncthreads();
    if (sh.stop) break;
  }
}

__global__ __launch_bounds__(S3_NT) void k_optimize_sim3(
    int cap, const int* __restrict__ d_count, const uint8_t* __restrict__ d_entry, const float* __restrict__ d_Xw1,
    const float* __restrict__ d_Xw2, const int* __restrict__ d_i2, const float* __restrict__ d_obs1, const float* __restrict__ d_inv1,
    const float* __restrict__ d_obs2, const float* __restrict__ d_inv2, const float* __restrict__ d_T1w, const float* __restrict__ d_T2w,
    const float* __restrict__ d_cam1, const float* __restrict__ d_cam2, const float* __restrict__ d_th2, const uint8_t* __restrict__ d_fix,
    int bAllPoints, double* __restrict__ d_S12, uint8_t* __restrict__ d_keep, int* __restrict__ d_nIn, int* __restrict__ d_stats,
    char* __restrict__ ws, size_t wsPitch) {
  __shared__ S3Shared sh;
  const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int n = d_count ? min(max(d_count[p], 0), cap) : cap;
  const S3Work w = s3_carve(ws + (size_t)p * wsPitch, cap);
  const size_t pc = (size_t)p * cap;
  Camera c1, c2;
  c1.kb8 = d_cam1[p * 9] != 0.f; c2.kb8 = d_cam2[p * 9] != 0.f;
  for (int i = 0; i < 8; ++i) { c1.p[i] = d_cam1[p * 9 + 1 + i]; c2.p[i] = d_cam2[p * 9 + 1 + i]; }
  float T1[12], T2[12];
  for (int i = 0; i < 12; ++i) { T1[i] = d_T1w[p * 12 + i]; T2[i] = d_T2w[p * 12 + i]; }
  const float th2 = d_th2[p];
  const bool fixScale = d_fix[p] != 0;
  const double delta = (double)sqrtf(th2);   // const float deltaHuber = sqrt(th2)

  for (int i = t; i < cap; i += S3_NT) d_keep[pc + i] = (i < n && (d_entry[pc + i] & 1)) ? 1 : 0;
  if (t == 0) {
    sh.nc = 0;
    for (int i = 0; i < 4; ++i) sh.S.q[i] = d_S12[p * 8 + i];
    for (int i = 0; i < 3; ++i) sh.S.t[i] = d_S12[p * 8 + 4 + i];
    sh.S.s = d_S12[p * 8 + 7];
  }
  __syncthreads();
  // ---- the edge set (:2118-2231), compacted in feature order ----
  for (int base = 0; base < n; base += S3_NT) {
    const int i = base + t;
    bool valid = false;
    float P1[3], P2[3];
    if (i < n) {
      const uint8_t en = d_entry[pc + i];
      // bit 0 matched, bit 1 pMP1 present, bit 2 pMP1 bad, bit 3 pMP2 bad
      if ((en & 1) && (en & 2) && !(en & 4) && !(en & 8)) {
        const int i2 = d_i2[pc + i];
        if (!(i2 < 0 && !bAllPoints)) {
          const float* X1 = d_Xw1 + (pc + i) * 3;
          const float* X2 = d_Xw2 + (pc + i) * 3;
          for (int r = 0; r < 3; ++r) {
            P1[r] = T1[r * 3] * X1[0] + T1[r * 3 + 1] * X1[1] + T1[r * 3 + 2] * X1[2] + T1[9 + r];
            P2[r] = T2[r * 3] * X2[0] + T2[r * 3 + 1] * X2[1] + T2[r * 3 + 2] * X2[2] + T2[9 + r];
          }
          valid = !(P2[2] < 0);
        }
      }
    }
    const unsigned long long bal = __ballot(valid);
    const int below = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) sh.wcount[wv] = __popcll(bal);
    __syncthreads();
    int off = sh.nc;
    for (int k = 0; k < wv; ++k) off += sh.wcount[k];
    if (valid) {
      const int c = off + below;
      double* cr = w.corr + (size_t)c * S3_CORR;
      for (int r = 0; r < 3; ++r) { cr[r] = (double)P2[r]; cr[3 + r] = (double)P1[r]; }
      cr[6] = (double)d_obs1[(pc + i) * 2]; cr[7] = (double)d_obs1[(pc + i) * 2 + 1];
      if (d_i2[pc + i] >= 0) {
        cr[8] = (double)d_obs2[(pc + i) * 2]; cr[9] = (double)d_obs2[(pc + i) * 2 + 1];
      } else {   // the normalised coordinates of P3D2c stand in for a keypoint (the reference's pixel-vs-normalised quirk)
        const float invz = 1 / P2[2];
        const float x = P2[0] * invz, y = P2[1] * invz;
        cr[8] = (double)x; cr[9] = (double)y;
      }
      cr[10] = (double)d_inv1[pc + i];
      cr[11] = (double)d_inv2[pc + i];
      w.idx[c] = i;
      w.act[c] = 1;
    }
    __syncthreads();
    if (t == 0) { int tot = 0; for (int k = 0; k < S3_NT / 64; ++k) tot += sh.wcount[k]; sh.nc += tot; }
    __syncthreads();
  }
  const int nc = sh.nc;
  const int E2 = 2 * cap;
  int it1 = 0, tr1 = 0, it2 = 0, tr2 = 0, reached = 0;
  // ---- phase 1: optimize(5) with Huber kernels ----
  if (nc > 0) {
    lm_optimize(sh, w, E2, 5, true, delta, fixScale, c1, c2);
    it1 = sh.iters; tr1 = sh.trials;
  }
  if (t == 0) { sh.nBad1 = 0; sh.nIn = 0; }
  __syncthreads();
  // inlier check on the chi2 of the last evaluated errors (:2237-2259)
  for (int c = t; c < nc; c += S3_NT) {
    if (w.chi[2 * c] > (double)th2 || w.chi[2 * c + 1] > (double)th2) {
      w.act[c] = 0;
      d_keep[pc + w.idx[c]] = 0;
      atomicAdd(&sh.nBad1, 1);
    }
  }
  __syncthreads();
  const int nBad = sh.nBad1;
  if (nc - nBad >= 10) {
    // ---- phase 2: inliers only, no robust kernel ----
    lm_optimize(sh, w, E2, nBad > 0 ? 10 : 5, false, delta, fixScale, c1, c2);
    it2 = sh.iters; tr2 = sh.trials;
    eval_edges<false>(w, nc, E2, sh.S, false, delta, fixScale, c1, c2);
    __syncthreads();
    for (int c = t; c < nc; c += S3_NT) {
      if (!w.act[c]) continue;
      if (w.chi[2 * c] > (double)th2 || w.chi[2 * c + 1] > (double)th2) d_keep[pc + w.idx[c]] = 0;
      else atomicAdd(&sh.nIn, 1);
    }
    __syncthreads();
    reached = 1;
    if (t == 0) {
      for (int i = 0; i < 4; ++i) d_S12[p * 8 + i] = sh.S.q[i];
      for (int i = 0; i < 3; ++i) d_S12[p * 8 + 4 + i] = sh.S.t[i];
      d_S12[p * 8 + 7] = sh.S.s;
    }
  }
  if (t == 0) {
    d_nIn[p] = reached ? sh.nIn : 0;
    int* st = d_stats + (size_t)p * 8;
    st[0] = it1; st[1] = tr1; st[2] = it2; st[3] = tr2; st[4] = reached; st[5] = nc; st[6] = nBad; st[7] = reached ? sh.nIn : 0;
  }
}

}  // namespace

extern "C" int morb_optimize_sim3_batch(morb_optimizer* o, int nprob, int cap, const int* d_count, const uint8_t* d_entry,
                                        const float* d_Xw1, const float* d_Xw2, const int* d_i2, const float* d_obs1,
                                        const float* d_invSigma2_1, const float* d_obs2, const float* d_invSigma2_2, const float* d_T1w,
                                        const float* d_T2w, const float* d_cam1, const float* d_cam2, const float* d_th2,
                                        const uint8_t* d_fixScale, int bAllPoints, double* d_S12, uint8_t* d_keep, int* d_nIn,
                                        int* d_stats, void* stream) {
  MORB_REQUIRE(o && d_entry && d_Xw1 && d_Xw2 && d_i2 && d_obs1 && d_invSigma2_1 && d_obs2 && d_invSigma2_2 && d_T1w && d_T2w && d_cam1 &&
                   d_cam2 && d_th2 && d_fixScale && d_S12 && d_keep && d_nIn && d_stats,
               MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nprob > 0 && cap > 0, MORB_ERR_INVALID, "bad sizes");
  MORB_ENTER(st, o, stream);
  const size_t pitch = s3_bytes_per_problem(cap);
  char* ws = nullptr;
  const int rc = morb::grow(o->spill, pitch * (size_t)nprob, &ws);
  if (rc != MORB_OK) return rc;
  hipLaunchKernelGGL(k_optimize_sim3, dim3(nprob), dim3(S3_NT), 0, st, cap, d_count, d_entry, d_Xw1, d_Xw2, d_i2, d_obs1, d_invSigma2_1,
                     d_obs2, d_invSigma2_2, d_T1w, d_T2w, d_cam1, d_cam2, d_th2, d_fixScale, bAllPoints, d_S12, d_keep, d_nIn, d_stats,
                     ws, pitch);
  MORB_HIP_CHECK(hipGetLastError());
  return MORB_OK;
}
