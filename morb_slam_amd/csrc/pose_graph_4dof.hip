// Optimizer::OptimizeEssentialGraph4DoF (reference src/Optimizer.cc:5163-5472) for MI355X (gfx950): the pose graph of loop closing in an
// inertial map, where gravity has made roll and pitch observable and a loop corrects yaw and translation only.  Vertices are VertexPose4DoF
// (G2oTypes.h:155-189): an ImuCamPose with four unknowns (yaw, tx, ty, tz) applied through UpdateW (G2oTypes.cc:218-248); edges are Edge4DoF
// (G2oTypes.h:816-842): a 6-vector on the camera poses, information diag(1e3, 1e3, 1, 1, 1, 1), no robust kernel.
//   * the vertex state (PG4_STATE doubles): Rcw, tcw, DR, twb and `its`; Rwb0 stays apart, Rcb / tcb are one calibration for the map.  At
//     entry Rcw / tcw are what the caller gives, independent of the body state: the first computeError reads them as given, and UpdateW
//     recomputes them from DR, Rwb0 and twb.  `its` counts accepted updates; at 5, after Rwb has been taken, DR(0,2), DR(1,2), DR(2,0),
//     DR(2,1) are zeroed (they act from the next update on) and `its` returns to 0.  NormalizeRotation(DR)'s result is discarded there by
//     the reference, so nothing stands for it here.  A rejected trial and a Jacobian's perturbation are undone by g2o's push / pop: the
//     trial states live in T, and the perturbed copies in registers.
//   * k_pg4_linearize: g2o's numeric Jacobians (base_binary_edge.hpp:131-205: central differences, delta = 1e-9, through oplusImpl on a
//     pushed copy), one lane per (edge, vertex, column): 16 computeError calls per edge and one for the error itself.
//   * k_pg4_assemble: constructQuadraticForm's non-robust branch, b += J^T (-Omega e), A += (J^T Omega) J, every 4 x 4 block and gradient
//     summed in edge insertion order over the lists of envelope_plan.h: no floating-point atomics.
//   * k_pg4_maxdiag: computeLambdaInit (optimization_algorithm_levenberg.cpp:171-185).  There is no setUserLambdaInit in this optimiser:
//     the first lambda is 1e-5 * max |H_jj| of the first assembled system, taken behind the first assembly and before the first factorisation.
//   * k_pg4_factor / k_pg4_backsub: the block LDL^T over the envelope of the 4 x 4 block rows and both substitutions (envelope_ldlt.h,
//     which describes the schedule).  A block is 128 bytes: PG4_STAGE of them are staged at a time, 64 covering rows take one pass, four
//     blocks' loads are kept in flight.  A pivot has to be positive.  The trial states UpdateW(x) follow the backward substitution.
//   * k_pg4_errors / k_pg4_decide: chi2 = e^T Omega e per edge, summed in edge order; g2o's Levenberg-Marquardt decisions (lm_control.h:
//     lm_decide_trial), optimize(20), no stop flag, the host queueing trials through ba_host.h's lm_slot_queue.
//   * k_pg4_finish: the point correction of :5451-5470.
// A vertex without an edge is not in g2o's active set: it is not in the system and keeps its bytes.
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
#include "inertial_device.h"
#include "internal_abi.h"
#include "lm_control.h"

namespace {

using namespace morb;

constexpr int PG4_NT = 256;                          // lanes of a workgroup: 64 covering rows of 4 lines in one pass of the factorisation
constexpr int PG4_STAGE = 128;                       // blocks of the column's own row envelope_factor stages in LDS at a time (16 KiB)
constexpr size_t PG4_MAX_BLOCKS = (size_t)1 << 22;   // envelope blocks a handle may grow to
constexpr int PG4_SUM = 2048;                        // values staged in LDS per pass of an ordered sum
constexpr int PG4_STATE = 28;                        // doubles of a vertex state: Rcw 0..8, tcw 9..11, DR 12..20, twb 21..23, its 24
constexpr double PG4_DELTA = 1e-9;                   // the step of g2o's numeric Jacobians

struct Pg4Dev {
  int nKF, nE, n, nBlocks, nMP, maxIts;
  const int *eI, *eJ;        // [nE]
  const double* eT;          // [nE][12] dRij row-major, dtij
  const uint8_t* fixed;      // [nKF]
  const int* col;            // [nKF] block row of the system, -1: fixed or without an edge
  const int *rowFirst, *rowOff, *colStart, *colRows, *listStart, *listItems;   // envelope_plan.h
  double *S, *T;             // [nKF][PG4_STATE] current and trial states
  const double* Rwb0;        // [nKF][9]
  const double* Scw;         // [nKF][8] vScw at entry (qx qy qz qw tx ty tz s), when nMP > 0
  double Rcb[9], tcb[3];
  double* J;                 // [nE][2][24] Jacobians, row-major (error component, unknown)
  double* err;               // [nE][6] error at S
  double* chiE;              // [nE] chi2 of the last computeError
  double *H, *L;             // [nBlocks][16] H in the envelope; its factor (strictly lower blocks, unit-lower diagonal blocks)
  double *b, *y, *x, *d;     // [4 n] right-hand side, work vector, solution, D of the factorisation
  LmControl* lm;
  double* chi2;              // [2] active chi2 before and after
  int* lmi;                  // [8] LMW_* (lm_control.h)
  int* lmHost;               // mapped host words: [0] decided trials, [1] done
  float* mp;                 // [nMP][3]
  const int* mpRef;          // [nMP]
};

__device__ __forceinline__ double pg4_omega(int k) { return k < 2 ? 1e3 : 1.0; }   // matLambda (Optimizer.cc:5231-5234)

// ImuCamPose::UpdateW({0, 0, u0, u1, u2, u3}) on a state in registers (G2oTypes.cc:218-248)
__device__ void pg4_update(double* s, const double* Rwb0, const double* Rcb, const double* tcb, const double* u) {
  const double ur[3] = {0.0, 0.0, u[0]};
  double dR[9], Rwb[9], Rbw[9], tbw[3];
  exp_so3(ur, dR);
  mul33(dR, s + 12, s + 12);   // DR = dR * DR
  mul33(s + 12, Rwb0, Rwb);
#pragma unroll
  for (int k = 0; k < 3; ++k) s[21 + k] += u[1 + k];
  s[24] += 1.0;
  if (s[24] >= 5.0) {
    s[12 + 2] = 0.0; s[12 + 5] = 0.0; s[12 + 6] = 0.0; s[12 + 7] = 0.0;
    s[24] = 0.0;
  }
  transpose33(Rwb, Rbw);
  mul3v(Rbw, s + 21, tbw);
#pragma unroll
  for (int k = 0; k < 3; ++k) tbw[k] = -tbw[k];
  mul33(Rcb, Rbw, s);
  mul3v(Rcb, tbw, s + 9);
#pragma unroll
  for (int k = 0; k < 3; ++k) s[9 + k] += tcb[k];
}

// Edge4DoF::computeError on the camera poses (Rcw, tcw: the first 12 doubles of a state)
__device__ void pg4_error(const double* M, const double* Pi, const double* Pj, double* e) {
  double RjT[9], dRT[9], A[9], v[3];
  transpose33(Pj, RjT);
  transpose33(M, dRT);
  mul33(Pi, RjT, A);
  mul33(A, dRT, A);
  log_so3(A, e);
  mul3v(RjT, Pj + 9, v);
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = -v[k];
  mul3v(Pi, v, v);
#pragma unroll
  for (int k = 0; k < 3; ++k) e[3 + k] = v[k] + Pi[9 + k] - M[9 + k];
}

__device__ __forceinline__ void pg4_load(const double* p, double* s) {
#pragma unroll
  for (int k = 0; k < 25; ++k) s[k] = p[k];
}

// linearizeOplus of every edge at S: lanes 0 .. 3 of an edge's 16 take the columns of vertex 0, 4 .. 7 those of vertex 1, 8 the error
__global__ __launch_bounds__(PG4_NT) void k_pg4_linearize(Pg4Dev D) {
  if (D.lmi[LMW_DONE] || !D.lmi[LMW_REBUILD]) return;
  const int gid = blockIdx.x * PG4_NT + threadIdx.x;
  const int e = gid >> 4, k = gid & 15;
  if (e >= D.nE || k >= 9) return;
  const int vi = D.eI[e], vj = D.eJ[e];
  const double* M = D.eT + (size_t)e * 12;
  const double *Pi = D.S + (size_t)vi * PG4_STATE, *Pj = D.S + (size_t)vj * PG4_STATE;
  if (k == 8) {
    double er[6];
    pg4_error(M, Pi, Pj, er);
#pragma unroll
    for (int r = 0; r < 6; ++r) D.err[(size_t)e * 6 + r] = er[r];
    return;
  }
  const int side = k >> 2, d = k & 3;
  const int v = side ? vj : vi;
  if (D.fixed[v]) return;   // (a fixed vertex has no Jacobian)
  double sp[25], sm[25], u[4], ep[6], em[6];
  pg4_load(D.S + (size_t)v * PG4_STATE, sp);
  pg4_load(D.S + (size_t)v * PG4_STATE, sm);
#pragma unroll
  for (int i = 0; i < 4; ++i) u[i] = i == d ? PG4_DELTA : 0.0;
  pg4_update(sp, D.Rwb0 + (size_t)v * 9, D.Rcb, D.tcb, u);
#pragma unroll
  for (int i = 0; i < 4; ++i) u[i] = i == d ? -PG4_DELTA : 0.0;
  pg4_update(sm, D.Rwb0 + (size_t)v * 9, D.Rcb, D.tcb, u);
  if (side) { pg4_error(M, Pi, sp, ep); pg4_error(M, Pi, sm, em); }
  else { pg4_error(M, sp, Pj, ep); pg4_error(M, sm, Pj, em); }
  const double scalar = 1.0 / (2 * PG4_DELTA);
  double* J = D.J + ((size_t)e * 2 + side) * 24;
#pragma unroll
  for (int r = 0; r < 6; ++r) J[r * 4 + d] = scalar * (ep[r] - em[r]);
}

// H in the envelope and b, every entry summed over its contributions in edge order
__global__ __launch_bounds__(PG4_NT) void k_pg4_assemble(Pg4Dev D) {
  if (D.lmi[LMW_DONE] || !D.lmi[LMW_REBUILD]) return;
  const size_t gid = (size_t)blockIdx.x * PG4_NT + threadIdx.x;
  const size_t nH = (size_t)D.nBlocks * 16;
  if (gid < nH) {
    const int blk = (int)(gid >> 4), r = (int)(gid >> 2) & 3, c = (int)gid & 3;
    double acc = 0;
    for (int q = D.listStart[blk]; q < D.listStart[blk + 1]; ++q) {
      const int it = D.listItems[q], e = it >> 2, kind = it & 3;
      // rows: the Jacobian of the block's row vertex; columns: that of its column vertex
      const double* Jr = D.J + ((size_t)e * 2 + (kind & 1)) * 24;
      const double* Jc = D.J + ((size_t)e * 2 + (kind < 2 ? (kind & 1) : 1 - (kind & 1))) * 24;
      double v = 0;
#pragma unroll
      for (int k = 0; k < 6; ++k) v += (Jr[k * 4 + r] * pg4_omega(k)) * Jc[k * 4 + c];
      acc += v;
    }
    D.H[gid] = acc;
    return;
  }
  const size_t g = gid - nH;
  if (g >= (size_t)D.n * 4) return;
  const int a = (int)(g >> 2), r = (int)g & 3;
  const int blk = D.rowOff[a + 1] - 1;   // the diagonal block's list names every edge of the vertex
  double acc = 0;
  for (int q = D.listStart[blk]; q < D.listStart[blk + 1]; ++q) {
    const int it = D.listItems[q], e = it >> 2;
    const double* Jr = D.J + ((size_t)e * 2 + (it & 1)) * 24;
    const double* er = D.err + (size_t)e * 6;
    double v = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) v += Jr[k * 4 + r] * (-(pg4_omega(k) * er[k]));
    acc += v;
  }
  D.b[g] = acc;
}

// computeLambdaInit behind the first assembly: 1e-5 * max |H_jj| over the vertices of the system.  One workgroup; a maximum has no order.
__global__ __launch_bounds__(PG4_NT) void k_pg4_maxdiag(Pg4Dev D) {
  __shared__ double sMax[PG4_NT];
  if (D.lmi[LMW_DONE] || !D.lmi[LMW_LAMBDA0]) return;
  const int t = threadIdx.x;
  double m = 0;
  for (int i = t; i < 4 * D.n; i += PG4_NT) {
    const int a = i >> 2, r = i & 3;
    m = fmax(m, fabs(D.H[((size_t)D.rowOff[a + 1] - 1) * 16 + r * 5]));
  }
  sMax[t] = m;
  __syncthreads();
  for (int w = PG4_NT / 2; w > 0; w >>= 1) {
    if (t < w) sMax[t] = fmax(sMax[t], sMax[t + w]);
    __syncthreads();
  }
  if (t == 0) {
    LmControl c = *D.lm;
    lm_begin(c, 0.0, sMax[0]);
    *D.lm = c;
    D.lmi[LMW_LAMBDA0] = 0;
  }
}

// H + lambda I = L D L^T over the envelope, and y = L^-1 b on the way (envelope_ldlt.h).  One workgroup.  A pivot has to be positive: the
// reference's Cholesky fails otherwise.
__global__ __launch_bounds__(PG4_NT) void k_pg4_factor(Pg4Dev D) {
  if (D.lmi[LMW_DONE]) return;
  const bool ok = envelope_factor<4, PG4_NT, PG4_STAGE, 4, true>(envelope_sys(D), D.lm->lambda);
  if (threadIdx.x == 0) D.lmi[LMW_OK2] = ok ? 1 : 0;
}

// x = L^-T D^-1 y (envelope_ldlt.h), then the trial states UpdateW(x_v).  One workgroup.
__global__ __launch_bounds__(PG4_NT) void k_pg4_backsub(Pg4Dev D) {
  if (D.lmi[LMW_DONE]) return;
  const int t = threadIdx.x;
  if (D.lmi[LMW_OK2]) envelope_backsub<4, PG4_NT>(envelope_sys(D));
  // ---- the trial states (a failed factorisation leaves x as it was: g2o still applies it) ----
  for (int v = t; v < D.nKF; v += PG4_NT) {
    const int a = D.col[v];
    double s[25];
    pg4_load(D.S + (size_t)v * PG4_STATE, s);
    if (a >= 0) {
      double u[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) u[k] = D.x[(size_t)a * 4 + k];
      pg4_update(s, D.Rwb0 + (size_t)v * 9, D.Rcb, D.tcb, u);
    }
#pragma unroll
    for (int k = 0; k < 25; ++k) D.T[(size_t)v * PG4_STATE + k] = s[k];
  }
}

// computeError of every edge at the trial states (trial != 0) or at S
__global__ __launch_bounds__(PG4_NT) void k_pg4_errors(Pg4Dev D, int trial) {
  if (D.lmi[LMW_DONE]) return;
  const int e = blockIdx.x * PG4_NT + threadIdx.x;
  if (e >= D.nE) return;
  const double* X = trial ? D.T : D.S;
  double er[6];
  pg4_error(D.eT + (size_t)e * 12, X + (size_t)D.eI[e] * PG4_STATE, X + (size_t)D.eJ[e] * PG4_STATE, er);
  double chi = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) chi += er[k] * (pg4_omega(k) * er[k]);
  D.chiE[e] = chi;
}

// init != 0: behind the first computeActiveErrors; else g2o's decision after a trial (lm_control.h).  One workgroup.
__global__ __launch_bounds__(PG4_NT) void k_pg4_decide(Pg4Dev D, int init) {
  __shared__ double buf[PG4_SUM];
  __shared__ int sKeep;
  if (D.lmi[LMW_DONE]) return;
  const int t = threadIdx.x;
  const double chi = lm_sum_in_index_order<PG4_NT, PG4_SUM>(buf, D.nE, [&](int e) { return D.chiE[e]; });
  LmControl c = *D.lm;
  if (init) {
    if (t == 0) {
      lm_iteration(c, chi);   // (lambda comes behind the first assembly: k_pg4_maxdiag)
      *D.lm = c;
      D.chi2[0] = chi; D.chi2[1] = chi;
      D.lmi[LMW_REBUILD] = 1; D.lmi[LMW_ITS] = 0; D.lmi[LMW_TRIALS] = 0; D.lmi[LMW_OK2] = 1; D.lmi[LMW_LAMBDA0] = 1;
    }
    return;
  }
  const double lambda = c.lambda;
  const double gain = lm_sum_in_index_order<PG4_NT, PG4_SUM>(buf, 4 * D.n, [&](int i) { return D.x[i] * (lambda * D.x[i] + D.b[i]); });   // computeScale()
  if (t == 0) sKeep = lm_decide_trial(c, chi, D.lmi[LMW_OK2] != 0, gain, false, D.maxIts, D.lm, D.chi2, D.lmi, D.lmHost) ? 1 : 0;
  __syncthreads();
  if (sKeep)
    for (int i = t; i < PG4_STATE * D.nKF; i += PG4_NT) D.S[i] = D.T[i];
}

__device__ __forceinline__ void pg4_qrot(const double* q, const double* v, double* o) {   // QuaternionBase::_transformVector
  const double ux = q[0], uy = q[1], uz = q[2], w = q[3];
  double a = uy * v[2] - uz * v[1], b = uz * v[0] - ux * v[2], c = ux * v[1] - uy * v[0];
  a += a; b += b; c += c;
  o[0] = v[0] + w * a + (uy * c - uz * b);
  o[1] = v[1] + w * b + (uz * a - ux * c);
  o[2] = v[2] + w * c + (ux * b - uy * a);
}

// the point correction (:5451-5470): correctedSwr.map(Srw.map(P)) in FP64, then float; correctedSwr = (Ri, ti, 1)^-1
__global__ __launch_bounds__(PG4_NT) void k_pg4_finish(Pg4Dev D) {
  const int m = blockIdx.x * PG4_NT + threadIdx.x;
  if (m >= D.nMP) return;
  const int v = D.mpRef[m];
  if (v < 0) return;
  const double* Srw = D.Scw + (size_t)v * 8;
  const double* P = D.S + (size_t)v * PG4_STATE;
  const double X[3] = {(double)D.mp[m * 3], (double)D.mp[m * 3 + 1], (double)D.mp[m * 3 + 2]};
  double a[3], RT[9], o[3];
  pg4_qrot(Srw, X, a);
#pragma unroll
  for (int k = 0; k < 3; ++k) a[k] = Srw[7] * a[k] + Srw[4 + k] - P[9 + k];
  transpose33(P, RT);
  mul3v(RT, a, o);
  for (int k = 0; k < 3; ++k) D.mp[m * 3 + k] = (float)o[k];
}

}  // namespace

extern "C" int morb_optimize_essential_graph_4dof(morb_optimizer* o, int nKF, double* kfPose, const double* kfBody, const uint8_t* kfFixed,
                                                  const float* Tcb12, int nE, const int* eI, const int* eJ, const double* eTij, int nMP,
                                                  float* mpPos, const int* mpRef, const double* kfScw, int* stats4, double* chi2) {
  MORB_REQUIRE(o && kfPose && kfBody && kfFixed && Tcb12 && stats4 && chi2 && (nE == 0 || (eI && eJ && eTij)) && (nMP == 0 || (mpPos && mpRef && kfScw)),
               MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nKF > 0 && nE >= 0 && nMP >= 0, MORB_ERR_INVALID, "bad sizes");   // (nE = 0: no free vertex has an edge, below)
  auto finite = [](const double* p, size_t n) {
    for (size_t k = 0; k < n; ++k) if (!std::isfinite(p[k])) return false;
    return true;
  };
  MORB_REQUIRE(finite(kfPose, (size_t)12 * nKF) && finite(kfBody, (size_t)12 * nKF), MORB_ERR_INVALID, "a non-finite pose or body state");
  for (int k = 0; k < 12; ++k) MORB_REQUIRE(std::isfinite(Tcb12[k]), MORB_ERR_INVALID, "a non-finite calibration");
  for (int e = 0; e < nE; ++e) {
    MORB_REQUIRE(eI[e] >= 0 && eI[e] < nKF && eJ[e] >= 0 && eJ[e] < nKF, MORB_ERR_INVALID, "edge index out of range");
    MORB_REQUIRE(eI[e] != eJ[e], MORB_ERR_INVALID, "an edge joins a vertex to itself");
  }
  MORB_REQUIRE(nE == 0 || finite(eTij, (size_t)12 * nE), MORB_ERR_INVALID, "a non-finite measurement");
  for (int m = 0; m < nMP; ++m) MORB_REQUIRE(mpRef[m] >= -1 && mpRef[m] < nKF, MORB_ERR_INVALID, "point reference out of range");
  if (nMP) {
    MORB_REQUIRE(finite(kfScw, (size_t)8 * nKF), MORB_ERR_INVALID, "a non-finite Sim3 at entry");
    for (int v = 0; v < nKF; ++v) MORB_REQUIRE(kfScw[(size_t)v * 8 + 7] > 0, MORB_ERR_INVALID, "a Sim3 at entry with a scale <= 0");
  }
  std::vector<uint8_t> fixed(nKF);
  for (int v = 0; v < nKF; ++v) fixed[v] = kfFixed[v] ? 1 : 0;
  EnvelopePlan P;
  const EnvelopeFit fit = plan_envelope(nKF, fixed.data(), nE, eI, eJ, PG4_MAX_BLOCKS, P);
  if (fit == EnvelopeFit::Empty) {   // no free vertex has an edge: nothing to optimise, nothing written
    for (int k = 0; k < 4; ++k) stats4[k] = 0;
    chi2[0] = chi2[1] = 0;
    return MORB_OK;
  }
  MORB_REQUIRE(fit == EnvelopeFit::Ok, MORB_ERR_CAPACITY, "the envelope of the 4-DoF pose graph exceeds what the handle may grow to");
  const int n = P.n, nBlocks = P.nBlocks;
  // the states at entry: Rcw, tcw as given; DR = I, twb, its = 0; Rwb0 apart
  std::vector<double> state((size_t)PG4_STATE * nKF, 0.0), Rwb0((size_t)9 * nKF);
  for (int v = 0; v < nKF; ++v) {
    double* s = state.data() + (size_t)v * PG4_STATE;
    memcpy(s, kfPose + (size_t)v * 12, sizeof(double) * 12);
    s[12] = s[16] = s[20] = 1.0;
    memcpy(s + 21, kfBody + (size_t)v * 12 + 9, sizeof(double) * 3);
    memcpy(Rwb0.data() + (size_t)v * 9, kfBody + (size_t)v * 12, sizeof(double) * 9);
  }

  MORB_ENTER(st, o, nullptr);
  Pg4Dev D;
  memset(&D, 0, sizeof D);
  D.nKF = nKF; D.nE = nE; D.n = n; D.nBlocks = nBlocks; D.nMP = nMP; D.maxIts = 20;
  for (int k = 0; k < 9; ++k) D.Rcb[k] = (double)Tcb12[k];
  for (int k = 0; k < 3; ++k) D.tcb[k] = (double)Tcb12[9 + k];
  ArenaCarver A;
  auto carve = [&]() {
    D.eI = (const int*)A.take(eI, sizeof(int) * nE); D.eJ = (const int*)A.take(eJ, sizeof(int) * nE);
    D.eT = (const double*)A.take(eTij, sizeof(double) * 12 * nE);
    D.fixed = (const uint8_t*)A.take(fixed.data(), nKF); D.col = (const int*)A.take(P.col.data(), sizeof(int) * nKF);
    D.rowFirst = (const int*)A.take(P.rowFirst.data(), sizeof(int) * n); D.rowOff = (const int*)A.take(P.rowOff.data(), sizeof(int) * (n + 1));
    D.colStart = (const int*)A.take(P.colStart.data(), sizeof(int) * (n + 1));
    D.colRows = (const int*)A.take(P.colRows.data(), sizeof(int) * P.colRows.size());
    D.listStart = (const int*)A.take(P.listStart.data(), sizeof(int) * P.listStart.size());
    D.listItems = (const int*)A.take(P.listItems.data(), sizeof(int) * P.listItems.size());
    D.S = (double*)A.take(state.data(), sizeof(double) * PG4_STATE * nKF);
    D.Rwb0 = (const double*)A.take(Rwb0.data(), sizeof(double) * 9 * nKF);
    if (nMP) {
      D.mp = (float*)A.take(mpPos, sizeof(float) * 3 * nMP); D.mpRef = (const int*)A.take(mpRef, sizeof(int) * nMP);
      D.Scw = (const double*)A.take(kfScw, sizeof(double) * 8 * nKF);
    }
    D.T = (double*)A.take(nullptr, sizeof(double) * PG4_STATE * nKF);
    D.J = (double*)A.take(nullptr, sizeof(double) * 48 * nE); D.err = (double*)A.take(nullptr, sizeof(double) * 6 * nE);
    D.chiE = (double*)A.take(nullptr, sizeof(double) * nE);
    D.H = (double*)A.take(nullptr, sizeof(double) * 16 * (size_t)nBlocks); D.L = (double*)A.take(nullptr, sizeof(double) * 16 * (size_t)nBlocks);
    D.b = (double*)A.take(nullptr, sizeof(double) * 4 * n); D.y = (double*)A.take(nullptr, sizeof(double) * 4 * n);
    D.x = (double*)A.take(nullptr, sizeof(double) * 4 * n); D.d = (double*)A.take(nullptr, sizeof(double) * 4 * n);
    D.lm = (LmControl*)A.take(nullptr, sizeof(LmControl)); D.chi2 = (double*)A.take(nullptr, sizeof(double) * 2);
    D.lmi = (int*)A.take(nullptr, sizeof(int) * 8);
  };
  carve();   // (dry: sizes)
  char *arena = nullptr, *stage = nullptr;
  { const int rc = grow(o->essentialGraph, A.uploadBytes() + A.deviceBytes(), &arena); if (rc != MORB_OK) return rc; }
  { const int rc = grow(o->stage, A.uploadBytes(), &stage); if (rc != MORB_OK) return rc; }
  A.bind(arena, stage);
  carve();
  if (!A.ok()) { set_error("the two carve passes of OptimizeEssentialGraph4DoF differ"); return MORB_ERR_HIP; }
  int *hostw = nullptr, *hostwDev = nullptr;
  MORB_REQUIRE(morb_optimizer_lm_words(o, &hostw, &hostwDev) == MORB_OK, MORB_ERR_HIP, "cannot map the LM state words");
  D.lmHost = hostwDev;
  reset_lm_words(hostw, 2, nullptr);
  MORB_HIP_CHECK(hipMemcpyAsync(arena, stage, A.uploadBytes(), hipMemcpyHostToDevice, st));   // the one upload
  // the workspace is reused from call to call (and shared with OptimizeEssentialGraph): what the first kernels expect to find zero is cleared
  MORB_HIP_CHECK(hipMemsetAsync(D.lmi, 0, sizeof(int) * 8, st));
  MORB_HIP_CHECK(hipMemsetAsync(D.lm, 0, sizeof(LmControl), st));
  MORB_HIP_CHECK(hipMemsetAsync(D.x, 0, sizeof(double) * 4 * n, st));   // the solver's x before the first solve
  MORB_HIP_CHECK(hipMemsetAsync(D.J, 0, sizeof(double) * 48 * nE, st));   // (the Jacobian of a fixed vertex is never written, and never read)

  const int edgeBlocks = div_up(nE, PG4_NT);
  const size_t asmItems = (size_t)nBlocks * 16 + (size_t)n * 4;
  hipLaunchKernelGGL(k_pg4_errors, dim3(edgeBlocks), dim3(PG4_NT), 0, st, D, 0);   // computeActiveErrors
  hipLaunchKernelGGL(k_pg4_decide, dim3(1), dim3(PG4_NT), 0, st, D, 1);
  MORB_HIP_CHECK(hipGetLastError());
  // a slot is one trial: at most 20 iterations of 10 trials
  const int q = lm_slot_queue(200, hostw + 0, hostw + 1, [&](int) {
    hipLaunchKernelGGL(k_pg4_linearize, dim3(div_up(nE * 16, PG4_NT)), dim3(PG4_NT), 0, st, D);   // (both run only behind an accepted trial)
    hipLaunchKernelGGL(k_pg4_assemble, dim3((unsigned)((asmItems + PG4_NT - 1) / PG4_NT)), dim3(PG4_NT), 0, st, D);
    hipLaunchKernelGGL(k_pg4_maxdiag, dim3(1), dim3(PG4_NT), 0, st, D);                           // (behind the first assembly only)
    hipLaunchKernelGGL(k_pg4_factor, dim3(1), dim3(PG4_NT), 0, st, D);
    hipLaunchKernelGGL(k_pg4_backsub, dim3(1), dim3(PG4_NT), 0, st, D);
    hipLaunchKernelGGL(k_pg4_errors, dim3(edgeBlocks), dim3(PG4_NT), 0, st, D, 1);
    hipLaunchKernelGGL(k_pg4_decide, dim3(1), dim3(PG4_NT), 0, st, D, 0);
    if (hipGetLastError() != hipSuccess) { set_error("OptimizeEssentialGraph4DoF: a trial's launch failed"); return (int)MORB_ERR_HIP; }
    return (int)MORB_OK;
  }, [&]() { return stream_look(st, "OptimizeEssentialGraph4DoF"); }, []() {});
  if (q < 0) return MORB_ERR_HIP;
  if (nMP) hipLaunchKernelGGL(k_pg4_finish, dim3(div_up(nMP, PG4_NT)), dim3(PG4_NT), 0, st, D);
  MORB_HIP_CHECK(hipGetLastError());
  int hi[8];
  std::vector<double> out((size_t)PG4_STATE * nKF);
  MORB_HIP_CHECK(hipMemcpyAsync(hi, D.lmi, sizeof hi, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipMemcpyAsync(chi2, D.chi2, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipMemcpyAsync(out.data(), D.S, sizeof(double) * PG4_STATE * nKF, hipMemcpyDeviceToHost, st));
  if (nMP) MORB_HIP_CHECK(hipMemcpyAsync(mpPos, D.mp, sizeof(float) * 3 * nMP, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipStreamSynchronize(st));   // (also drains a queue that ran out of slots before the words are reset again)
  for (int v = 0; v < nKF; ++v) memcpy(kfPose + (size_t)v * 12, out.data() + (size_t)v * PG4_STATE, sizeof(double) * 12);
  stats4[0] = hi[LMW_ITS]; stats4[1] = hi[LMW_TRIALS]; stats4[2] = n; stats4[3] = nBlocks;
  return MORB_OK;
}
