// Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:1443-1735, and the graph of :1737-2063) for MI355X (gfx950): the Sim3 pose
// graph of loop closing on the flattened graph.  Vertices are g2o::Sim3 estimates with a `fixed` and a `_fix_scale` flag each; edges are
// EdgeSim3 (error log(Sji * Si * Sj^-1), types_seven_dof_expmap.h:106-114, information = identity, no robust kernel).
//   * k_eg_linearize: the numeric Jacobians as BaseBinaryEdge::linearizeOplus takes them (base_binary_edge.hpp:131-205: central differences,
//     delta = 1e-9, through VertexSim3Expmap::oplusImpl, which zeroes update[6] of a vertex with _fix_scale), one lane per (edge, vertex,
//     column): 28 computeError calls per edge, grid-wide.  Sim3::log (types/sim3.h:148-230) with its eps branches on sigma and d and its
//     3 x 3 partial-pivot LU; the product, inverse and exponential are sim3_math.h's, shared with OptimizeSim3.
//   * k_eg_assemble: BaseBinaryEdge::constructQuadraticForm's non-robust branch.  Every 7 x 7 block and gradient is summed in edge
//     insertion order over per-block lists (ba_host.h: csr_by_key), one lane per entry: no floating-point atomics.  A fixed endpoint
//     contributes no block and no gradient; a scale column of a _fix_scale vertex is exactly zero and stays in the system (diagonal =
//     lambda, right-hand side 0).
//   * k_eg_factor: the block-sparse LDL^T.  7 unknowns per vertex over the whole map and no points to eliminate: in the caller's vertex order
//     the matrix is a block band (spanning tree, covisibility) plus a few long rows (loop edges), which the block envelope of
//     envelope_plan.h holds with its fill.  The factorisation is envelope_ldlt.h's, which describes storage and schedule: 36 covering rows
//     take one pass, EG_PANEL blocks of the column's own row are staged at a time, four blocks' loads are kept in flight.  H + lambda I is
//     positive definite or the trial fails (ok2 = false), as the reference's Cholesky does.
//   * k_eg_backsub: the backward substitution (envelope_ldlt.h), and the trial estimates exp(x) * S behind it.
//   * k_eg_errors / k_eg_decide: the trial's chi2 per edge, summed in edge order by one lane; g2o's Levenberg-Marquardt decisions
//     (lm_control.h: lm_decide_trial) with setUserLambdaInit(1e-16) and optimize(20) on the device, the host queueing trials through
//     ba_host.h's lm_slot_queue.
//   * k_eg_finish: the point correction of :1707-1731 behind the solve.
//   * k_egm_prepare / k_egm_finish: the second overload (map merging, :1737-2063) around the same solve.  Before it, the float poses of the
//     three lists become g2o::Sim3 estimates in FP64 and every kept edge gets its measurement by the reference's good / bad rules; after
//     it, the SE3 recovery, the float inverse, the BefMerge copies and the float SE3 point correction of :2015-2062.  The two entries
//     share the carve of the solver's arrays and the launch sequence (eg_carve_plan, eg_carve_solver, eg_solve).
// A vertex without an edge is not in g2o's active set: it is not in the system and keeps its bytes.  A free component with no path to a
// fixed vertex is gauge-free; it is neither detected nor repaired here (lambda keeps the factorisation defined, as it does in g2o).
// acos and log inside Sim3::log are the device library's (tests/test_essential_graph_gpu.py measures them against the host libm).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ba_host.h"
#include "common.h"
#include "envelope_ldlt.h"
#include "envelope_plan.h"
#include "handles.h"
#include "internal_abi.h"
#include "lm_control.h"
#include "sim3_math.h"

namespace {

using namespace morb;

constexpr int EG_NT = 256;
constexpr int EG_PANEL = 32;                    // blocks of the column's own row envelope_factor stages in LDS at a time
constexpr size_t EG_MAX_BLOCKS = (size_t)1 << 22;   // envelope blocks a handle may grow to (matrix and factor: 2 x 1.5 GiB)
constexpr int EG_SUM = 2048;                    // values staged in LDS per pass of an ordered sum

struct EgDev {
  int nKF, nE, n, nBlocks, nMP, maxIts;
  const int *eI, *eJ;        // [nE]
  const double* eS;          // [nE][8] measurement Sji
  const uint8_t* flags;      // [nKF] bit 0 fixed, bit 1 _fix_scale
  const int* col;            // [nKF] block row of the system, -1: fixed or without an edge
  const int* rowFirst;       // [n] first block column of row i's envelope
  const int* rowOff;         // [n + 1] envelope block of (i, rowFirst[i])
  const int* colStart;       // [n + 1] the rows below j whose envelope covers column j: colRows[colStart[j] .. colStart[j + 1]), ascending
  const int* colRows;
  const int* listStart;      // [nBlocks + 1] contributions of envelope block k, in edge order
  const int* listItems;      // edge * 4 + kind: 0 / 1 diagonal block of vertex 0 / 1, 2 / 3 off-diagonal block whose row is vertex 0 / 1
  double *S, *T;             // [nKF][8] current and trial estimates (qx qy qz qw tx ty tz s)
  const double* S0;          // [nKF][8] the estimates at entry
  double* J;                 // [nE][2][49] Jacobians, row-major (error component, unknown)
  double* err;               // [nE][7] error at S
  double* chiE;              // [nE] chi2 of the last computeError
  double *H, *L;             // [nBlocks][49] H in the envelope; its factor (strictly lower blocks, unit-lower diagonal blocks)
  double *b, *y, *x, *d;     // [7 n] right-hand side, work vector, solution, D of the factorisation
  LmControl* lm;
  double* chi2;              // [2] active chi2 before and after
  int* lmi;                  // [8] LMW_* (lm_control.h)
  int* lmHost;               // mapped host words: [0] decided trials, [1] done
  float* mp;                 // [nMP][3]
  const int* mpRef;          // [nMP]
};

__device__ __forceinline__ Sim3d eg_load(const double* p) {
  Sim3d s;
  for (int i = 0; i < 4; ++i) s.q[i] = p[i];
  for (int i = 0; i < 3; ++i) s.t[i] = p[4 + i];
  s.s = p[7];
  return s;
}
__device__ __forceinline__ void eg_store(double* p, const Sim3d& s) {
  for (int i = 0; i < 4; ++i) p[i] = s.q[i];
  for (int i = 0; i < 3; ++i) p[4 + i] = s.t[i];
  p[7] = s.s;
}

// Sim3::log (types/sim3.h:148-230).  W.lu().solve(t) is Eigen's PartialPivLU of a 3 x 3 matrix: the row swaps are written out so that no
// array is indexed by a run-time value.
__device__ void sim3_log(const Sim3d& S, double* res) {
  const double sigma = log(S.s);
  const double x = S.q[0], y = S.q[1], z = S.q[2], w = S.q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;   // Quaterniond::toRotationMatrix
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  const double R00 = 1 - (tyy + tzz), R01 = txy - twz, R02 = txz + twy, R10 = txy + twz, R11 = 1 - (txx + tzz), R12 = tyz - twx,
               R20 = txz - twy, R21 = tyz + twx, R22 = 1 - (txx + tyy);
  const double d = 0.5 * (R00 + R11 + R22 - 1);
  const double dR[3] = {R21 - R12, R02 - R20, R10 - R01};   // deltaR(R)
  const double eps = 0.00001;
  double A, B, C, om[3];
  if (fabs(sigma) < eps) {
    C = 1;
    if (d > 1 - eps) {
      for (int i = 0; i < 3; ++i) om[i] = 0.5 * dR[i];
      A = 1. / 2.; B = 1. / 6.;
    } else {
      const double theta = acos(d);
      const double theta2 = theta * theta;
      const double f = theta / (2 * sqrt(1 - d * d));
      for (int i = 0; i < 3; ++i) om[i] = f * dR[i];
      A = (1 - morbm64::cos_glibc(theta)) / (theta2);
      B = (theta - morbm64::sin_glibc(theta)) / (theta2 * theta);
    }
  } else {
    C = (S.s - 1) / sigma;
    if (d > 1 - eps) {
      const double sigma2 = sigma * sigma;
      for (int i = 0; i < 3; ++i) om[i] = 0.5 * dR[i];
      A = ((sigma - 1) * S.s + 1) / (sigma2);
      B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
    } else {
      const double theta = acos(d);
      const double f = theta / (2 * sqrt(1 - d * d));
      for (int i = 0; i < 3; ++i) om[i] = f * dR[i];
      const double theta2 = theta * theta;
      const double a = S.s * morbm64::sin_glibc(theta);
      const double b = S.s * morbm64::cos_glibc(theta);
      const double c = theta2 + sigma * sigma;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  const double Om[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
  double W[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double o2 = Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j] + Om[i * 3 + 2] * Om[6 + j];
      W[i * 3 + j] = A * Om[i * 3 + j] + B * o2 + C * (i == j ? 1.0 : 0.0);
    }
  // PartialPivLU, rows a0 a1 a2 with their right-hand sides
  double a0[4] = {W[0], W[1], W[2], S.t[0]}, a1[4] = {W[3], W[4], W[5], S.t[1]}, a2[4] = {W[6], W[7], W[8], S.t[2]};
  auto swap4 = [](double* p, double* q) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { const double v = p[i]; p[i] = q[i]; q[i] = v; }
  };
  {
    int p = 0;
    double big = fabs(a0[0]);
    if (fabs(a1[0]) > big) { big = fabs(a1[0]); p = 1; }
    if (fabs(a2[0]) > big) { big = fabs(a2[0]); p = 2; }
    if (p == 1) swap4(a0, a1); else if (p == 2) swap4(a0, a2);
  }
  a1[0] /= a0[0]; a2[0] /= a0[0];
  a1[1] -= a1[0] * a0[1]; a1[2] -= a1[0] * a0[2];
  a2[1] -= a2[0] * a0[1]; a2[2] -= a2[0] * a0[2];
  if (fabs(a2[1]) > fabs(a1[1])) swap4(a1, a2);
  a2[1] /= a1[1];
  a2[2] -= a2[1] * a1[2];
  const double y0 = a0[3], y1 = a1[3] - a1[0] * y0, y2 = a2[3] - (a2[0] * y0 + a2[1] * y1);
  const double u2 = y2 / a2[2];
  const double u1 = (y1 - a1[2] * u2) / a1[1];
  const double u0 = (y0 - (a0[1] * u1 + a0[2] * u2)) / a0[0];
  res[0] = om[0]; res[1] = om[1]; res[2] = om[2];
  res[3] = u0; res[4] = u1; res[5] = u2;
  res[6] = sigma;
}

// EdgeSim3::computeError: log(C * v1 * v2^-1)
__device__ __forceinline__ void eg_error(const Sim3d& M, const Sim3d& Si, const Sim3d& Sj, double* e) {
  sim3_log(sim3_mul(sim3_mul(M, Si), sim3_inverse(Sj)), e);
}
// VertexSim3Expmap::oplusImpl with the update +-delta e_d (d in 0 .. 6), written without a run-time index; exp(+-1e-9) is glibc's (libm_f64.h)
__device__ __forceinline__ Sim3d eg_perturbed(const Sim3d& S, int d, bool plus, bool fixScale) {
  double u[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) u[i] = i == d ? (plus ? S3_DELTA : -S3_DELTA) : 0.0;
  if (fixScale) u[6] = 0;
  return sim3_mul(sim3_exp(u, u[6] == 0 ? 1.0 : morbm64::exp_glibc(u[6])), S);
}

// linearizeOplus of every edge at S: lanes 0 .. 6 of an edge's 16 take the columns of vertex 0, 7 .. 13 those of vertex 1, 14 the error
__global__ __launch_bounds__(EG_NT) void k_eg_linearize(EgDev D) {
  if (D.lmi[LMW_DONE] || !D.lmi[LMW_REBUILD]) return;
  const int gid = blockIdx.x * EG_NT + threadIdx.x;
  const int e = gid >> 4, k = gid & 15;
  if (e >= D.nE || k >= 15) return;
  const int vi = D.eI[e], vj = D.eJ[e];
  const Sim3d M = eg_load(D.eS + (size_t)e * 8), Si = eg_load(D.S + (size_t)vi * 8), Sj = eg_load(D.S + (size_t)vj * 8);
  if (k == 14) {
    double er[7];
    eg_error(M, Si, Sj, er);
#pragma unroll
    for (int r = 0; r < 7; ++r) D.err[(size_t)e * 7 + r] = er[r];
    return;
  }
  const int side = k >= 7 ? 1 : 0, d = k - 7 * side;
  const uint8_t fl = D.flags[side ? vj : vi];
  if (fl & 1) return;   // (a fixed vertex has no Jacobian)
  const bool fixScale = (fl & 2) != 0;
  const Sim3d Sp = eg_perturbed(side ? Sj : Si, d, true, fixScale), Sm = eg_perturbed(side ? Sj : Si, d, false, fixScale);
  double ep[7], em[7];
  if (side) { eg_error(M, Si, Sp, ep); eg_error(M, Si, Sm, em); }
  else { eg_error(M, Sp, Sj, ep); eg_error(M, Sm, Sj, em); }
  const double scalar = 1.0 / (2 * S3_DELTA);
  double* J = D.J + ((size_t)e * 2 + side) * 49;
#pragma unroll
  for (int r = 0; r < 7; ++r) J[r * 7 + d] = scalar * (ep[r] - em[r]);
}

// H in the envelope and b, every entry summed over its contributions in edge order
__global__ __launch_bounds__(EG_NT) void k_eg_assemble(EgDev D) {
  if (D.lmi[LMW_DONE] || !D.lmi[LMW_REBUILD]) return;
  const size_t gid = (size_t)blockIdx.x * EG_NT + threadIdx.x;
  const size_t nH = (size_t)D.nBlocks * 49;
  if (gid < nH) {
    const int blk = (int)(gid / 49), ent = (int)(gid % 49), r = ent / 7, c = ent % 7;
    double acc = 0;
    for (int q = D.listStart[blk]; q < D.listStart[blk + 1]; ++q) {
      const int it = D.listItems[q], e = it >> 2, kind = it & 3;
      // rows: the Jacobian of the block's row vertex; columns: that of its column vertex
      const double* Jr = D.J + ((size_t)e * 2 + (kind & 1)) * 49;
      const double* Jc = D.J + ((size_t)e * 2 + (kind < 2 ? (kind & 1) : 1 - (kind & 1))) * 49;
      double v = 0;
#pragma unroll
      for (int k = 0; k < 7; ++k) v += Jr[k * 7 + r] * Jc[k * 7 + c];
      acc += v;
    }
    D.H[gid] = acc;
    return;
  }
  const size_t g = gid - nH;
  if (g >= (size_t)D.n * 7) return;
  const int a = (int)(g / 7), r = (int)(g % 7);
  const int blk = D.rowOff[a + 1] - 1;   // the diagonal block's list names every edge of the vertex
  double acc = 0;
  for (int q = D.listStart[blk]; q < D.listStart[blk + 1]; ++q) {
    const int it = D.listItems[q], e = it >> 2;
    const double* Jr = D.J + ((size_t)e * 2 + (it & 1)) * 49;
    const double* er = D.err + (size_t)e * 7;
    double v = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) v += Jr[k * 7 + r] * (-er[k]);
    acc += v;
  }
  D.b[g] = acc;
}

// H + lambda I = L D L^T over the envelope, and y = L^-1 b on the way (envelope_ldlt.h).  One workgroup.  A pivot has to be positive, as
// the reference's Cholesky asks.
__global__ __launch_bounds__(EG_NT) void k_eg_factor(EgDev D) {
  if (D.lmi[LMW_DONE]) return;
  const bool ok = envelope_factor<7, EG_NT, EG_PANEL, 4, true>(envelope_sys(D), D.lm->lambda);
  if (threadIdx.x == 0) D.lmi[LMW_OK2] = ok ? 1 : 0;
}

// x = L^-T D^-1 y: row i, once final, is taken out of the rows above it; then the trial estimates exp(x_v) * S_v.  One workgroup.
// The 7 x 7 substitution keeps a schedule of its own instead of envelope_ldlt.h's envelope_backsub: the next row's diagonal block (392
// bytes) is fetched into LDS by 49 idle lanes while the others scatter the current row, so lane 0's serial solve never waits for global
// memory.  Measured (profiles/r23): 4.74 ms per call at 500 keyframes and 24.0 ms at 2000 against 5.53 and 27.4 on the shared body.
__global__ __launch_bounds__(EG_NT) void k_eg_backsub(EgDev D) {
  __shared__ double sLb[2][49], sx[7];
  if (D.lmi[LMW_DONE]) return;
  const int t = threadIdx.x, n = D.n;
  if (D.lmi[LMW_OK2]) {
    for (int i = t; i < 7 * n; i += EG_NT) D.x[i] = D.y[i] / D.d[i];
    if (t >= 192 && t < 241) sLb[(n - 1) & 1][t - 192] = D.L[((size_t)D.rowOff[n] - 1) * 49 + t - 192];
    __threadfence_block();
    __syncthreads();
    for (int i = n - 1; i >= 0; --i) {
      const int fi = D.rowFirst[i];
      const size_t rowI = (size_t)D.rowOff[i];
      if (t == 0) {   // x_i = L_ii^-T z_i
        const double* sL = sLb[i & 1];
        double z[7], xx[7];
#pragma unroll
        for (int r = 0; r < 7; ++r) z[r] = D.x[(size_t)i * 7 + r];
#pragma unroll
        for (int r = 6; r >= 0; --r) {
          double v = z[r];
#pragma unroll
          for (int p = r + 1; p < 7; ++p) v -= sL[p * 7 + r] * xx[p];
          xx[r] = v;
        }
#pragma unroll
        for (int r = 0; r < 7; ++r) { sx[r] = xx[r]; D.x[(size_t)i * 7 + r] = xx[r]; }
      }
      __syncthreads();
      if (i > 0 && t >= 192 && t < 241) sLb[(i - 1) & 1][t - 192] = D.L[((size_t)D.rowOff[i] - 1) * 49 + t - 192];   // the next row's diagonal block
      const int cnt = (i - fi) * 7;
      for (int item = t; item < cnt; item += EG_NT) {
        const int kk = item / 7, c = item - 7 * kk;
        const double* lik = D.L + (rowI + kk) * 49;
        double dot = 0;
#pragma unroll
        for (int r = 0; r < 7; ++r) dot += lik[r * 7 + c] * sx[r];
        D.x[(size_t)(fi + kk) * 7 + c] -= dot;
      }
      __threadfence_block();
      __syncthreads();
    }
  }
  // ---- the trial estimates (a failed factorisation leaves x as it was: g2o still applies it) ----
  for (int v = t; v < D.nKF; v += EG_NT) {
    const int a = D.col[v];
    Sim3d S = eg_load(D.S + (size_t)v * 8);
    if (a >= 0) {
      double u[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) u[k] = D.x[(size_t)a * 7 + k];
      if (D.flags[v] & 2) u[6] = 0;
      // (|u[6]| >= 512 would overflow the scale anyway: there the device library's exp)
      S = sim3_mul(sim3_exp(u, fabs(u[6]) < 512.0 ? morbm64::exp_glibc(u[6]) : exp(u[6])), S);
    }
    eg_store(D.T + (size_t)v * 8, S);
  }
}

// computeError of every edge at the trial estimates (trial != 0) or at S
__global__ __launch_bounds__(EG_NT) void k_eg_errors(EgDev D, int trial) {
  if (D.lmi[LMW_DONE]) return;
  const int e = blockIdx.x * EG_NT + threadIdx.x;
  if (e >= D.nE) return;
  const double* X = trial ? D.T : D.S;
  double er[7];
  eg_error(eg_load(D.eS + (size_t)e * 8), eg_load(X + (size_t)D.eI[e] * 8), eg_load(X + (size_t)D.eJ[e] * 8), er);
  double chi = 0;
#pragma unroll
  for (int k = 0; k < 7; ++k) chi += er[k] * er[k];
  D.chiE[e] = chi;
}

// init != 0: behind the first computeActiveErrors; else g2o's decision after a trial (lm_control.h).  One workgroup.
__global__ __launch_bounds__(EG_NT) void k_eg_decide(EgDev D, int init) {
  __shared__ double buf[EG_SUM];
  __shared__ int sKeep;
  if (D.lmi[LMW_DONE]) return;
  const int t = threadIdx.x;
  const double chi = lm_sum_in_index_order<EG_NT, EG_SUM>(buf, D.nE, [&](int e) { return D.chiE[e]; });
  LmControl c = *D.lm;
  if (init) {
    if (t == 0) {
      lm_begin(c, 1e-16, 0.0);   // setUserLambdaInit(1e-16)
      lm_iteration(c, chi);
      *D.lm = c;
      D.chi2[0] = chi; D.chi2[1] = chi;
      D.lmi[LMW_REBUILD] = 1; D.lmi[LMW_ITS] = 0; D.lmi[LMW_TRIALS] = 0; D.lmi[LMW_OK2] = 1;
    }
    return;
  }
  const double lambda = c.lambda;
  const double gain = lm_sum_in_index_order<EG_NT, EG_SUM>(buf, 7 * D.n, [&](int i) { return D.x[i] * (lambda * D.x[i] + D.b[i]); });   // computeScale()
  if (t == 0) sKeep = lm_decide_trial(c, chi, D.lmi[LMW_OK2] != 0, gain, false, D.maxIts, D.lm, D.chi2, D.lmi, D.lmHost) ? 1 : 0;
  __syncthreads();
  if (sKeep)
    for (int i = t; i < 8 * D.nKF; i += EG_NT) D.S[i] = D.T[i];
}

// the point correction (:1707-1731): correctedSwr.map(Srw.map(P)) in FP64, then float
__global__ __launch_bounds__(EG_NT) void k_eg_finish(EgDev D) {
  const int m = blockIdx.x * EG_NT + threadIdx.x;
  if (m >= D.nMP) return;
  const int v = D.mpRef[m];
  if (v < 0) return;
  const Sim3d Srw = eg_load(D.S0 + (size_t)v * 8), Swr = sim3_inverse(eg_load(D.S + (size_t)v * 8));
  const double P[3] = {(double)D.mp[m * 3], (double)D.mp[m * 3 + 1], (double)D.mp[m * 3 + 2]};
  double a[3], o[3];
  sim3_map(Srw, P, a);
  sim3_map(Swr, a, o);
  for (int k = 0; k < 3; ++k) D.mp[m * 3 + k] = (float)o[k];
}

// acos(d[i]) and log(s[i]) as sim3_log computes them
__global__ __launch_bounds__(EG_NT) void k_eg_libm(int n, const double* d, const double* s, double* acosOut, double* logOut) {
  const int i = blockIdx.x * EG_NT + threadIdx.x;
  if (i >= n) return;
  acosOut[i] = acos(d[i]);
  logOut[i] = log(s[i]);
}

// ---- map merging: the second overload (Optimizer.cc:1737-2063) around the same solve ----
// A vertex's list mask.  vpGoodPose = FIXED or CORRECTED, vpBadPose = CORRECTED or NONFIXED (:1806-1807, :1841-1842, :1872-1873); a vertex
// of CORRECTED | NONFIXED is the fixed-corrected one (sIdKF, :1850) that the tail of :2015-2030 still visits.
enum { MG_FIXED = 1, MG_CORRECTED = 2, MG_NONFIXED = 4 };

struct MgDev {
  int nKF, nE, nMP;
  const uint8_t* lists;      // [nKF] MG_*
  const float* in;           // [4][nKF][7] Tcw, Twc, TcwBefMerge, TwcBefMerge at entry: quaternion xyzw, translation
  float* out;                // [4][nKF][7] the same at exit, and [nMP][3] the points at exit behind them
  const int *eI, *eJ;        // [nE] the kept edges
  double* eS;                // [nE][8] their measurements
  double* S;                 // [nKF][8] the estimates
  const float* mp;           // [nMP][3] the points at entry
  const int* mpRef;          // [nMP]
};

struct Se3f { float q[4]; float t[3]; };   // Sophus::SE3f: unit quaternion x y z w, translation

// SO3(quaternion): coeffs() /= norm(), the squares summed as Eigen's four-wide reduction sums them, (x^2 + z^2) + (y^2 + w^2)
__device__ __forceinline__ void mg_normalize(double* q) {
  const double n = sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]));
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] /= n;
}
__device__ __forceinline__ void mg_normalize(float* q) {
  const float n = sqrtf((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]));
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] /= n;
}
// SO3f::operator*(point): uv = q.vec x p, uv += uv, p + w uv + q.vec x uv
__device__ __forceinline__ void mg_rotate(const float* q, const float* p, float* o) {
  float a = q[1] * p[2] - q[2] * p[1], b = q[2] * p[0] - q[0] * p[2], c = q[0] * p[1] - q[1] * p[0];
  a += a; b += b; c += c;
  o[0] = (p[0] + q[3] * a) + (q[1] * c - q[2] * b);
  o[1] = (p[1] + q[3] * b) + (q[2] * a - q[0] * c);
  o[2] = (p[2] + q[3] * c) + (q[0] * b - q[1] * a);
}
__device__ __forceinline__ Se3f mg_load(const float* p) {
  Se3f T;
#pragma unroll
  for (int k = 0; k < 4; ++k) T.q[k] = p[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) T.t[k] = p[4 + k];
  return T;
}
__device__ __forceinline__ void mg_store(float* p, const Se3f& T) {
#pragma unroll
  for (int k = 0; k < 4; ++k) p[k] = T.q[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) p[4 + k] = T.t[k];
}
// SE3f::inverse: invR = SO3f(q.conjugate()), which normalises; SE3f(invR, invR * (t * -1))
__device__ __forceinline__ Se3f mg_inverse(const Se3f& T) {
  Se3f r;
  r.q[0] = -T.q[0]; r.q[1] = -T.q[1]; r.q[2] = -T.q[2]; r.q[3] = T.q[3];
  mg_normalize(r.q);
  const float v[3] = {T.t[0] * -1.f, T.t[1] * -1.f, T.t[2] * -1.f};
  mg_rotate(r.q, v, r.t);
  return r;
}
// SE3f::operator*: SO3f(a.q * b.q), which normalises; a.t + a.so3 * b.t
__device__ __forceinline__ Se3f mg_mul(const Se3f& A, const Se3f& B) {
  Se3f r;
  const float *a = A.q, *b = B.q;
  r.q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  r.q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  r.q[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  r.q[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  mg_normalize(r.q);
  float rt[3];
  mg_rotate(A.q, B.t, rt);
#pragma unroll
  for (int k = 0; k < 3; ++k) r.t[k] = A.t[k] + rt[k];
  return r;
}
// Sophus::SE3d T = pose.cast<double>() (SO3d(q.cast<double>()) normalises); g2o::Sim3(T.unit_quaternion(), T.translation(), 1.0)
__device__ __forceinline__ Sim3d mg_sim3_of(const float* p) {
  Sim3d S;
#pragma unroll
  for (int k = 0; k < 4; ++k) S.q[k] = (double)p[k];
  mg_normalize(S.q);
#pragma unroll
  for (int k = 0; k < 3; ++k) S.t[k] = (double)p[4 + k];
  S.s = 1.0;
  return S;
}
// :2022-2029: Sophus::SE3d Tiw(CorrectedSiw.rotation(), CorrectedSiw.translation() / s), Tiw.cast<float>()
__device__ __forceinline__ Se3f mg_se3_of(const Sim3d& S) {
  double q[4] = {S.q[0], S.q[1], S.q[2], S.q[3]};
  mg_normalize(q);
  Se3f T;
#pragma unroll
  for (int k = 0; k < 4; ++k) T.q[k] = (float)q[k];
  mg_normalize(T.q);
#pragma unroll
  for (int k = 0; k < 3; ++k) T.t[k] = (float)(S.t[k] / S.s);
  return T;
}

// Before the solve.  Lane v < nKF: the estimate Siw of vertex v (:1790-1794, :1820-1824, :1855-1859).  Lane nKF + e: the measurement of kept
// edge e, Sji = Sjw * Swi (:1892-1916): Swi = vScw[i]^-1 where i is bad and the default g2o::Sim3() otherwise; Sjw = vCorrectedSwc[j]^-1
// where both are good, else vScw[j].  vScw is the Sim3 of mTcwBefMerge on a fixed-corrected vertex and of the pose on a non-fixed one.
__global__ __launch_bounds__(EG_NT) void k_egm_prepare(MgDev D) {
  const int gid = blockIdx.x * EG_NT + threadIdx.x;
  if (gid < D.nKF) {
    eg_store(D.S + (size_t)gid * 8, mg_sim3_of(D.in + (size_t)gid * 7));
    return;
  }
  const int e = gid - D.nKF;
  if (e >= D.nE) return;
  const int i = D.eI[e], j = D.eJ[e];
  const int li = D.lists[i], lj = D.lists[j];
  const float* bef = D.in + (size_t)2 * D.nKF * 7;   // TcwBefMerge
  Sim3d Swi;
  Swi.q[0] = Swi.q[1] = Swi.q[2] = 0; Swi.q[3] = 1; Swi.t[0] = Swi.t[1] = Swi.t[2] = 0; Swi.s = 1;
  if (li & (MG_CORRECTED | MG_NONFIXED)) Swi = sim3_inverse(mg_sim3_of(((li & MG_CORRECTED) ? bef : D.in) + (size_t)i * 7));
  Sim3d Sjw;
  if ((li & (MG_FIXED | MG_CORRECTED)) && (lj & (MG_FIXED | MG_CORRECTED))) Sjw = sim3_inverse(sim3_inverse(mg_sim3_of(D.in + (size_t)j * 7)));
  else Sjw = mg_sim3_of(((lj & MG_CORRECTED) ? bef : D.in) + (size_t)j * 7);
  eg_store(D.eS + (size_t)e * 8, sim3_mul(Sjw, Swi));
}

// After the solve (:2015-2062).  Lane v < nKF: a vertex of vpNonFixedKFs gets mTcwBefMerge / mTwcBefMerge = the pose and its inverse at
// entry, SetPose(SE3d(q, t / s).cast<float>()) and mTwc = mTcw.inverse() in float; every other vertex keeps its four poses.  Lane nKF + m:
// a point whose reference keyframe is bad-flagged becomes (Twr * TwrBefMerge^-1) * P in float, with the values the vertex lanes write
// (recomputed here: no lane reads another's output).
__global__ __launch_bounds__(EG_NT) void k_egm_finish(MgDev D) {
  const int gid = blockIdx.x * EG_NT + threadIdx.x;
  const size_t plane = (size_t)D.nKF * 7;
  if (gid < D.nKF) {
    const size_t at = (size_t)gid * 7;
    if (D.lists[gid] & MG_NONFIXED) {
      const Se3f Tcw = mg_se3_of(eg_load(D.S + (size_t)gid * 8));
      mg_store(D.out + at, Tcw);
      mg_store(D.out + plane + at, mg_inverse(Tcw));
#pragma unroll
      for (int k = 0; k < 7; ++k) { D.out[2 * plane + at + k] = D.in[at + k]; D.out[3 * plane + at + k] = D.in[plane + at + k]; }
    } else {
#pragma unroll
      for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int a = 0; a < 4; ++a) D.out[a * plane + at + k] = D.in[a * plane + at + k];
    }
    return;
  }
  const int m = gid - D.nKF;
  if (m >= D.nMP) return;
  const int v = D.mpRef[m];
  const float P[3] = {D.mp[m * 3], D.mp[m * 3 + 1], D.mp[m * 3 + 2]};
  float* o = D.out + 4 * plane + (size_t)m * 3;
  const int l = v < 0 ? 0 : D.lists[v];
  if (!(l & (MG_CORRECTED | MG_NONFIXED))) {   // no reference, or (:2059) "a reference KF from another map": the point stays
    o[0] = P[0]; o[1] = P[1]; o[2] = P[2];
    return;
  }
  const size_t at = (size_t)v * 7;
  Se3f Twr, TwrBef;
  if (l & MG_NONFIXED) {
    Twr = mg_inverse(mg_se3_of(eg_load(D.S + (size_t)v * 8)));
    TwrBef = mg_load(D.in + plane + at);
  } else {
    Twr = mg_load(D.in + plane + at);
    TwrBef = mg_load(D.in + 3 * plane + at);
  }
  const Se3f T = mg_mul(Twr, mg_inverse(TwrBef));
  float r[3];
  mg_rotate(T.q, P, r);
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = r[k] + T.t[k];
}

// ---- the host side both entries share ----
// the graph lists of a plan, in the upload region
void eg_carve_plan(ArenaCarver& A, EgDev& D, const EnvelopePlan& P, const uint8_t* flags, const int* eI, const int* eJ) {
  D.eI = (const int*)A.take(eI, sizeof(int) * D.nE); D.eJ = (const int*)A.take(eJ, sizeof(int) * D.nE);
  D.flags = (const uint8_t*)A.take(flags, D.nKF); D.col = (const int*)A.take(P.col.data(), sizeof(int) * D.nKF);
  D.rowFirst = (const int*)A.take(P.rowFirst.data(), sizeof(int) * D.n); D.rowOff = (const int*)A.take(P.rowOff.data(), sizeof(int) * (D.n + 1));
  D.colStart = (const int*)A.take(P.colStart.data(), sizeof(int) * (D.n + 1)); D.colRows = (const int*)A.take(P.colRows.data(), sizeof(int) * P.colRows.size());
  D.listStart = (const int*)A.take(P.listStart.data(), sizeof(int) * P.listStart.size());
  D.listItems = (const int*)A.take(P.listItems.data(), sizeof(int) * P.listItems.size());
}
// the solver's own arrays, device only
void eg_carve_solver(ArenaCarver& A, EgDev& D) {
  const int nKF = D.nKF, nE = D.nE, n = D.n;
  D.T = (double*)A.take(nullptr, sizeof(double) * 8 * nKF);
  D.J = (double*)A.take(nullptr, sizeof(double) * 98 * nE); D.err = (double*)A.take(nullptr, sizeof(double) * 7 * nE);
  D.chiE = (double*)A.take(nullptr, sizeof(double) * nE);
  D.H = (double*)A.take(nullptr, sizeof(double) * 49 * (size_t)D.nBlocks); D.L = (double*)A.take(nullptr, sizeof(double) * 49 * (size_t)D.nBlocks);
  D.b = (double*)A.take(nullptr, sizeof(double) * 7 * n); D.y = (double*)A.take(nullptr, sizeof(double) * 7 * n);
  D.x = (double*)A.take(nullptr, sizeof(double) * 7 * n); D.d = (double*)A.take(nullptr, sizeof(double) * 7 * n);
  D.lm = (LmControl*)A.take(nullptr, sizeof(LmControl)); D.chi2 = (double*)A.take(nullptr, sizeof(double) * 2);
  D.lmi = (int*)A.take(nullptr, sizeof(int) * 8);
}
// the handle's block and its pinned mirror for a carve function, bound and carved
template <class Carve>
int eg_bind(morb_optimizer* o, ArenaCarver& A, Carve&& carve, char** arena, char** stage) {
  carve();   // (dry: sizes)
  { const int rc = grow(o->essentialGraph, A.uploadBytes() + A.deviceBytes(), arena); if (rc != MORB_OK) return rc; }
  { const int rc = grow(o->stage, A.uploadBytes(), stage); if (rc != MORB_OK) return rc; }
  A.bind(*arena, *stage);
  carve();
  if (!A.ok()) { set_error("the two carve passes of OptimizeEssentialGraph differ"); return MORB_ERR_HIP; }
  return MORB_OK;
}
// setUserLambdaInit(1e-16), optimize(20) on the uploaded graph: the clears, computeActiveErrors and the queue of trials
int eg_solve(morb_optimizer* o, hipStream_t st, EgDev& D) {
  const int nE = D.nE, n = D.n, nBlocks = D.nBlocks;
  int *hostw = nullptr, *hostwDev = nullptr;
  MORB_REQUIRE(morb_optimizer_lm_words(o, &hostw, &hostwDev) == MORB_OK, MORB_ERR_HIP, "cannot map the LM state words");
  D.lmHost = hostwDev;
  reset_lm_words(hostw, 2, nullptr);
  // the workspace is reused from call to call: what the first kernels expect to find zero is cleared behind the carve
  MORB_HIP_CHECK(hipMemsetAsync(D.lmi, 0, sizeof(int) * 8, st));
  MORB_HIP_CHECK(hipMemsetAsync(D.lm, 0, sizeof(LmControl), st));
  MORB_HIP_CHECK(hipMemsetAsync(D.x, 0, sizeof(double) * 7 * n, st));   // the solver's x before the first solve
  MORB_HIP_CHECK(hipMemsetAsync(D.J, 0, sizeof(double) * 98 * nE, st));   // (the Jacobian of a fixed vertex is never written, and never read)

  const int edgeBlocks = div_up(nE, EG_NT);
  const size_t asmItems = (size_t)nBlocks * 49 + (size_t)n * 7;
  hipLaunchKernelGGL(k_eg_errors, dim3(edgeBlocks), dim3(EG_NT), 0, st, D, 0);   // computeActiveErrors
  hipLaunchKernelGGL(k_eg_decide, dim3(1), dim3(EG_NT), 0, st, D, 1);
  MORB_HIP_CHECK(hipGetLastError());
  // a slot is one trial: at most 20 iterations of 10 trials
  const int q = lm_slot_queue(200, hostw + 0, hostw + 1, [&](int) {
    hipLaunchKernelGGL(k_eg_linearize, dim3(div_up(nE * 16, EG_NT)), dim3(EG_NT), 0, st, D);   // (both run only behind an accepted trial)
    hipLaunchKernelGGL(k_eg_assemble, dim3((unsigned)((asmItems + EG_NT - 1) / EG_NT)), dim3(EG_NT), 0, st, D);
    hipLaunchKernelGGL(k_eg_factor, dim3(1), dim3(EG_NT), 0, st, D);
    hipLaunchKernelGGL(k_eg_backsub, dim3(1), dim3(EG_NT), 0, st, D);
    hipLaunchKernelGGL(k_eg_errors, dim3(edgeBlocks), dim3(EG_NT), 0, st, D, 1);
    hipLaunchKernelGGL(k_eg_decide, dim3(1), dim3(EG_NT), 0, st, D, 0);
    if (hipGetLastError() != hipSuccess) { set_error("OptimizeEssentialGraph: a trial's launch failed"); return (int)MORB_ERR_HIP; }
    return (int)MORB_OK;
  }, [&]() { return stream_look(st, "OptimizeEssentialGraph"); }, []() {});
  return q < 0 ? MORB_ERR_HIP : MORB_OK;
}

}  // namespace

extern "C" int morb_optimize_essential_graph(morb_optimizer* o, int nKF, double* kfSim3, const uint8_t* kfFlags, int nE, const int* eI,
                                             const int* eJ, const double* eSji, int nMP, float* mpPos, const int* mpRef, int* stats4,
                                             double* chi2) {
  MORB_REQUIRE(o && kfSim3 && kfFlags && stats4 && chi2 && (nE == 0 || (eI && eJ && eSji)) && (nMP == 0 || (mpPos && mpRef)), MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nKF > 0 && nE >= 0 && nMP >= 0, MORB_ERR_INVALID, "bad sizes");   // (nE = 0: no free vertex has an edge, below)
  auto sound = [](const double* s) {
    for (int k = 0; k < 8; ++k) if (!std::isfinite(s[k])) return false;
    return s[7] > 0;
  };
  for (int v = 0; v < nKF; ++v) MORB_REQUIRE(sound(kfSim3 + (size_t)v * 8), MORB_ERR_INVALID, "a non-finite estimate or a scale <= 0");
  for (int e = 0; e < nE; ++e) {
    MORB_REQUIRE(eI[e] >= 0 && eI[e] < nKF && eJ[e] >= 0 && eJ[e] < nKF, MORB_ERR_INVALID, "edge index out of range");
    MORB_REQUIRE(eI[e] != eJ[e], MORB_ERR_INVALID, "an edge joins a vertex to itself");
    MORB_REQUIRE(sound(eSji + (size_t)e * 8), MORB_ERR_INVALID, "a non-finite measurement or a scale <= 0");
  }
  for (int m = 0; m < nMP; ++m) MORB_REQUIRE(mpRef[m] >= -1 && mpRef[m] < nKF, MORB_ERR_INVALID, "point reference out of range");
  EnvelopePlan P;
  const EnvelopeFit fit = plan_envelope(nKF, kfFlags, nE, eI, eJ, EG_MAX_BLOCKS, P);
  if (fit == EnvelopeFit::Empty) {   // no free vertex has an edge: nothing to optimise, nothing written
    for (int k = 0; k < 4; ++k) stats4[k] = 0;
    chi2[0] = chi2[1] = 0;
    return MORB_OK;
  }
  MORB_REQUIRE(fit == EnvelopeFit::Ok, MORB_ERR_CAPACITY, "the envelope of the essential graph exceeds what the handle may grow to");
  const int n = P.n, nBlocks = P.nBlocks;

  MORB_ENTER(st, o, nullptr);
  EgDev D;
  memset(&D, 0, sizeof D);
  D.nKF = nKF; D.nE = nE; D.n = n; D.nBlocks = nBlocks; D.nMP = nMP; D.maxIts = 20;
  ArenaCarver A;
  char *arena = nullptr, *stage = nullptr;
  {
    const int rc = eg_bind(o, A, [&]() {
      eg_carve_plan(A, D, P, kfFlags, eI, eJ);
      D.eS = (const double*)A.take(eSji, sizeof(double) * 8 * nE);
      D.S = (double*)A.take(kfSim3, sizeof(double) * 8 * nKF); D.S0 = (const double*)A.take(kfSim3, sizeof(double) * 8 * nKF);
      if (nMP) { D.mp = (float*)A.take(mpPos, sizeof(float) * 3 * nMP); D.mpRef = (const int*)A.take(mpRef, sizeof(int) * nMP); }
      eg_carve_solver(A, D);
    }, &arena, &stage);
    if (rc != MORB_OK) return rc;
  }
  MORB_HIP_CHECK(hipMemcpyAsync(arena, stage, A.uploadBytes(), hipMemcpyHostToDevice, st));   // the one upload
  { const int rc = eg_solve(o, st, D); if (rc != MORB_OK) return rc; }
  if (nMP) hipLaunchKernelGGL(k_eg_finish, dim3(div_up(nMP, EG_NT)), dim3(EG_NT), 0, st, D);
  MORB_HIP_CHECK(hipGetLastError());
  int hi[8];
  MORB_HIP_CHECK(hipMemcpyAsync(hi, D.lmi, sizeof hi, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipMemcpyAsync(chi2, D.chi2, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipMemcpyAsync(kfSim3, D.S, sizeof(double) * 8 * nKF, hipMemcpyDeviceToHost, st));
  if (nMP) MORB_HIP_CHECK(hipMemcpyAsync(mpPos, D.mp, sizeof(float) * 3 * nMP, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipStreamSynchronize(st));   // (also drains a queue that ran out of slots before the words are reset again)
  stats4[0] = hi[LMW_ITS]; stats4[1] = hi[LMW_TRIALS]; stats4[2] = n; stats4[3] = nBlocks;
  return MORB_OK;
}

extern "C" int morb_optimize_essential_graph_merge(morb_optimizer* o, int nKF, const uint8_t* kfLists, float* kfTcw, float* kfTwc, float* kfTcwBefMerge,
                                                   float* kfTwcBefMerge, int nC, const int* cI, const int* cJ, uint8_t* cKept, int nMP, float* mpPos,
                                                   const int* mpRef, int* stats4, double* chi2) {
  MORB_REQUIRE(o && kfLists && kfTcw && kfTwc && kfTcwBefMerge && kfTwcBefMerge && stats4 && chi2 && (nC == 0 || (cI && cJ && cKept)) &&
               (nMP == 0 || (mpPos && mpRef)), MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nKF > 0 && nC >= 0 && nMP >= 0, MORB_ERR_INVALID, "bad sizes");
  auto sound = [](const float* p) {   // finite, and a quaternion that SO3's constructor can normalise
    for (int k = 0; k < 7; ++k) if (!std::isfinite(p[k])) return false;
    return p[0] != 0 || p[1] != 0 || p[2] != 0 || p[3] != 0;
  };
  for (int v = 0; v < nKF; ++v) {
    const int l = kfLists[v];
    MORB_REQUIRE(l == MG_FIXED || l == MG_CORRECTED || l == MG_NONFIXED || l == (MG_CORRECTED | MG_NONFIXED), MORB_ERR_INVALID,
                 "a vertex is in no list, or in vpFixedKFs and another one");
    MORB_REQUIRE(sound(kfTcw + (size_t)v * 7) && sound(kfTwc + (size_t)v * 7), MORB_ERR_INVALID, "a non-finite pose or a zero quaternion");
    if (l & MG_CORRECTED)
      MORB_REQUIRE(sound(kfTcwBefMerge + (size_t)v * 7) && sound(kfTwcBefMerge + (size_t)v * 7), MORB_ERR_INVALID,
                   "a non-finite pose before the merge or a zero quaternion");
  }
  for (int c = 0; c < nC; ++c) {
    MORB_REQUIRE(cI[c] >= 0 && cI[c] < nKF && cJ[c] >= 0 && cJ[c] < nKF, MORB_ERR_INVALID, "edge index out of range");
    MORB_REQUIRE(cI[c] != cJ[c], MORB_ERR_INVALID, "an edge joins a vertex to itself");
  }
  for (int m = 0; m < nMP; ++m) MORB_REQUIRE(mpRef[m] >= -1 && mpRef[m] < nKF, MORB_ERR_INVALID, "point reference out of range");
  // the good / bad rule (:1907-1913): an edge exists where both ends are good or both are bad; fixed = every list but vpNonFixedKFs alone
  std::vector<uint8_t> flags(nKF), kept(nC);
  std::vector<int> eI, eJ;
  for (int v = 0; v < nKF; ++v) flags[v] = kfLists[v] == MG_NONFIXED ? 0 : (kfLists[v] == MG_FIXED ? 3 : 1);
  for (int c = 0; c < nC; ++c) {
    const int li = kfLists[cI[c]], lj = kfLists[cJ[c]];
    const bool good = (li & (MG_FIXED | MG_CORRECTED)) && (lj & (MG_FIXED | MG_CORRECTED));
    const bool bad = (li & (MG_CORRECTED | MG_NONFIXED)) && (lj & (MG_CORRECTED | MG_NONFIXED));
    kept[c] = good || bad;
    if (kept[c]) { eI.push_back(cI[c]); eJ.push_back(cJ[c]); }
  }
  const int nE = (int)eI.size();
  EnvelopePlan P;
  const EnvelopeFit fit = plan_envelope(nKF, flags.data(), nE, eI.data(), eJ.data(), EG_MAX_BLOCKS, P);
  MORB_REQUIRE(fit != EnvelopeFit::TooLarge, MORB_ERR_CAPACITY, "the envelope of the essential graph exceeds what the handle may grow to");
  const bool solve = fit == EnvelopeFit::Ok;   // (else no free vertex has an edge: the tail of :2015-2062 still runs)

  MORB_ENTER(st, o, nullptr);
  EgDev D;
  MgDev M;
  memset(&D, 0, sizeof D); memset(&M, 0, sizeof M);
  D.nKF = M.nKF = nKF; D.nE = M.nE = solve ? nE : 0; D.n = P.n; D.nBlocks = solve ? P.nBlocks : 0; D.nMP = M.nMP = nMP; D.maxIts = 20;
  const size_t plane = (size_t)7 * nKF;
  std::vector<float> in(4 * plane);   // the four poses of every vertex, plane by plane
  float* const host[4] = {kfTcw, kfTwc, kfTcwBefMerge, kfTwcBefMerge};
  for (int a = 0; a < 4; ++a) memcpy(in.data() + a * plane, host[a], sizeof(float) * plane);
  ArenaCarver A;
  char *arena = nullptr, *stage = nullptr;
  {
    const int rc = eg_bind(o, A, [&]() {
      M.lists = (const uint8_t*)A.take(kfLists, nKF);
      M.in = (const float*)A.take(in.data(), sizeof(float) * 4 * plane);
      if (nMP) { M.mp = (const float*)A.take(mpPos, sizeof(float) * 3 * nMP); M.mpRef = (const int*)A.take(mpRef, sizeof(int) * nMP); }
      if (solve) eg_carve_plan(A, D, P, flags.data(), eI.data(), eJ.data());
      M.out = (float*)A.take(nullptr, sizeof(float) * (4 * plane + (size_t)3 * nMP));
      D.S = M.S = (double*)A.take(nullptr, sizeof(double) * 8 * nKF);
      if (solve) { M.eS = (double*)A.take(nullptr, sizeof(double) * 8 * nE); D.eS = M.eS; eg_carve_solver(A, D); }
    }, &arena, &stage);
    if (rc != MORB_OK) return rc;
  }
  M.eI = D.eI; M.eJ = D.eJ;
  MORB_HIP_CHECK(hipMemcpyAsync(arena, stage, A.uploadBytes(), hipMemcpyHostToDevice, st));   // the one upload
  hipLaunchKernelGGL(k_egm_prepare, dim3(div_up(nKF + M.nE, EG_NT)), dim3(EG_NT), 0, st, M);
  MORB_HIP_CHECK(hipGetLastError());
  int hi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double hchi[2] = {0, 0};
  if (solve) {
    const int rc = eg_solve(o, st, D);
    if (rc != MORB_OK) return rc;
    MORB_HIP_CHECK(hipMemcpyAsync(hi, D.lmi, sizeof hi, hipMemcpyDeviceToHost, st));
    MORB_HIP_CHECK(hipMemcpyAsync(hchi, D.chi2, sizeof hchi, hipMemcpyDeviceToHost, st));
  }
  hipLaunchKernelGGL(k_egm_finish, dim3(div_up(nKF + nMP, EG_NT)), dim3(EG_NT), 0, st, M);
  MORB_HIP_CHECK(hipGetLastError());
  std::vector<float> out(4 * plane + (size_t)3 * nMP);   // the one download: the four planes and the points behind them
  MORB_HIP_CHECK(hipMemcpyAsync(out.data(), M.out, sizeof(float) * out.size(), hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipStreamSynchronize(st));   // (also drains a queue that ran out of slots before the words are reset again)
  for (int a = 0; a < 4; ++a) memcpy(host[a], out.data() + a * plane, sizeof(float) * plane);
  if (nMP) memcpy(mpPos, out.data() + 4 * plane, sizeof(float) * 3 * nMP);
  if (nC) memcpy(cKept, kept.data(), nC);
  stats4[0] = hi[LMW_ITS]; stats4[1] = hi[LMW_TRIALS]; stats4[2] = solve ? P.n : 0; stats4[3] = solve ? P.nBlocks : 0;
  chi2[0] = hchi[0]; chi2[1] = hchi[1];
  return MORB_OK;
}

extern "C" int morb_sim3_log_libm(morb_optimizer* o, int n, const double* d, const double* s, double* acosOut, double* logOut) {
  MORB_REQUIRE(o && d && s && acosOut && logOut && n > 0, MORB_ERR_INVALID, "bad argument");
  MORB_ENTER(st, o, nullptr);
  double* w = nullptr;
  { const int rc = grow(o->essentialGraph, sizeof(double) * 4 * (size_t)n, &w); if (rc != MORB_OK) return rc; }
  MORB_HIP_CHECK(hipMemcpyAsync(w, d, sizeof(double) * n, hipMemcpyHostToDevice, st));
  MORB_HIP_CHECK(hipMemcpyAsync(w + n, s, sizeof(double) * n, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_eg_libm, dim3(div_up(n, EG_NT)), dim3(EG_NT), 0, st, n, (const double*)w, (const double*)(w + n), w + 2 * (size_t)n, w + 3 * (size_t)n);
  MORB_HIP_CHECK(hipGetLastError());
  MORB_HIP_CHECK(hipMemcpyAsync(acosOut, w + 2 * (size_t)n, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipMemcpyAsync(logOut, w + 3 * (size_t)n, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipStreamSynchronize(st));
  return MORB_OK;
}
