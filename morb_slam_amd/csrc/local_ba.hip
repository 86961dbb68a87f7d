// Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:1053-1441) for MI355X (gfx950), device-resident: g2o's
// OptimizationAlgorithmLevenberg (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-194) over
// BlockSolver_6_3 (core/block_solver.hpp:354-590) with the reference's edges (src/OptimizableTypes.cpp,
// g2o/types/types_six_dof_expmap.cpp), on the handle of optimizer.hip and the device helpers of optimizer_device.h, in two modes:
//   * Grid mode (default): one launch per LM phase over the whole chip.  Hpp blocks per keyframe by a
//     wave per 64-edge chunk, Hll per map point by a thread; the Schur complement of the landmarks is ONE dense FP64 product
//     WD^T W on the matrix cores (schur_mfma.h: v_mfma_f64_16x16x4_f64, split-K with fixed-order partial sums); the reduced
//     camera system is factorised in LDS (dense_ldlt.h); back-substitution per map point.  The LM control flow
//     (optimization_algorithm_levenberg.cpp:61-169: rho, lambda schedule, <= 10 trials, the ORB-SLAM stop rule) runs ON THE
//     DEVICE in a one-workgroup decision kernel; every phase kernel reads the LM state and returns at once when the solve
//     is finished or the phase is not due, so the host only keeps the queue one trial ahead and watches a mapped flag.
//   * Persistent mode: one 1024-thread workgroup runs the whole loop (many small problems side by side).
// All arithmetic is FP64 like g2o; the reference's float leaks (float camera parameters, `const float invz` in
// the stereo projection, float Huber deltas, float chi2 tests) are reproduced.
// The welding bundle adjustment of map merging (Optimizer.cc:3430-3851: two rounds with an edge level between them) runs on the same graph,
// workspace and solver phases in grid mode; its own kernels (k_mg_*) and entry points are at the end of each half of this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "common.h"
#include "internal_abi.h"
#include "ba_host.h"
#include "dense_ldlt.h"
#include "schur_mfma.h"
#include "wave.h"
#include "optimizer_device.h"

using namespace morb;

namespace {

// =====================================================================================================
// LocalBundleAdjustment: one 1024-thread workgroup per problem
// =====================================================================================================
struct BaDev {
  int nKF, nMP, nE, nFree, P;           // P = 6 * nFree
  const int* kfCol;                     // [nKF] column of a free keyframe, -1 if fixed
  const int *eKF, *eMP;                 // [nE]
  const float *eObs, *eInfo;            // [nE][3], [nE]
  const int *mpStart, *mpEdges;         // CSR by map point
  const int *kfStart, *kfEdges;         // CSR by keyframe
  int nPairs;                           // upper-triangular block pairs (i1 <= i2) of the reduced system that occur
  const int *pairBlock;                 // [nPairs] i1 * nFree + i2
  const int *pairStart;                 // [nPairs + 1]
  const int2 *pairEntries;              // (e1, e2): two observations of one map point, col(e1) = i1, col(e2) = i2
  double *pose, *poseBk, *poseEval;     // [nKF][7]
  double *pt, *ptBk, *ptEval;           // [nMP][3]
  double *Hpp;                          // [nFree][36]
  double *Hll, *Dinv;                   // [nMP][9]
  double *Hpl;                          // [nE][18]
  double *b, *x;                        // [P + 3 nMP]
  double *HsG;                          // [P*P] global fallback for the reduced system
  float *poseIO, *ptIO;                 // results (float)
  uint8_t* erase;                       // [nE]
  int* stats;                           // [2]
  const int* stop;                      // device-visible abort flag (may be NULL)
  Cam cam;
  const struct Rig* rig;                // fisheye rig (KB8 cameras + mTrl) or NULL; its edges carry obs[2] = -2 (left camera) / -3 (right, "ToBody")
  double userLambda;
  // grid mode (one launch per LM phase across the whole chip)
  int nChunks;                          // keyframe edge lists cut into chunks of <= 64 edges (one wave each)
  const int *chunkKF, *chunkStart, *chunkEnd;   // [nChunks]
  const int *kfChunkStart;              // [nKF + 1]
  double *kfPart;                       // [nChunks][27]
  double *redPart;                      // [2][redBlocks] block partial sums (chi2, scale)
  double *scal;                         // [8] device scalars: chi2, scale, ok, maxdiag
  // device-side LM control (k_g_lm_*): the state of optimization_algorithm_levenberg.cpp's loop, and its mirror in mapped host memory
  double *lmd;                          // [4] LMD_*: currentChi, lambda, ni, iniChi
  int *lmi;                             // [16] LM_*
  int *lmHost;                          // [4] mapped host memory: decided trials, done, outer iterations, trials
  int *kfTicket;                        // [nKF] chunks of the keyframe that have delivered their partial blocks (k_g_build)
  int dupPairs;                         // some (keyframe, landmark) pair carries two edges (fisheye rig: both cameras)
  // Schur complement on the FP64 matrix cores (schur_mfma.h): dense K-major operands, partial products, block directory
  double *sW, *sWD, *sPart;
  const int2* sBlocks;
  const int* sBlkIndex;
  int sMp, sNb, sNblk, sNsplit;
};

__device__ __forceinline__ SE3 load_se3(const double* p) {
  SE3 s;
  for (int i = 0; i < 4; ++i) s.q[i] = p[i];
  for (int i = 0; i < 3; ++i) s.t[i] = p[4 + i];
  return s;
}
__device__ __forceinline__ void store_se3(double* p, const SE3& s) {
  for (int i = 0; i < 4; ++i) p[i] = s.q[i];
  for (int i = 0; i < 3; ++i) p[4 + i] = s.t[i];
}
__device__ __forceinline__ void inv3(const double* m, double* o) {
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double id = 1.0 / (m[0] * c00 + m[1] * c01 + m[2] * c02);
  o[0] = c00 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  o[3] = c01 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  o[6] = c02 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

constexpr int BA_T = 512, BA_W = BA_T / 64;

__global__ __launch_bounds__(BA_T) void k_local_ba(const BaDev* __restrict__ probs, int useLds) {
  extern __shared__ double sHs[];  // reduced camera system when it fits
  __shared__ double red[BA_W];
  __shared__ int sFlag;
  const BaDev pb = probs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int P = pb.P, nMP = pb.nMP, nE = pb.nE, nKF = pb.nKF;
  double* Hs = useLds ? sHs : pb.HsG;
  const double deltaMono = (double)(float)sqrt(5.991), deltaStereo = (double)(float)sqrt(7.815);
  const Cam cam = pb.cam;

  auto terminate = [&]() -> bool {
    if (!pb.stop) return false;
    __syncthreads();
    if (tid == 0) sFlag = __hip_atomic_load(pb.stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // host-written, pinned
    __syncthreads();
    return sFlag != 0;
  };
  // errors at the current estimate -> robust chi2; remembers the evaluation state (for the final chi2 test)
  auto chi2All = [&]() -> double {
    for (int i = tid; i < nKF * 7; i += BA_T) pb.poseEval[i] = pb.pose[i];
    for (int i = tid; i < nMP * 3; i += BA_T) pb.ptEval[i] = pb.pt[i];
    double s = 0;
    for (int e = tid; e < nE; e += BA_T) {
      const SE3 T = load_se3(pb.pose + 7 * pb.eKF[e]);
      double xc[3], err[3], w;
      se3_map(T, pb.pt + 3 * pb.eMP[e], xc);
      const float* o = pb.eObs + 3 * e;
      const bool st = !(o[2] < 0);
      const double c = ba_edge_error(cam, pb.rig, st, xc, o, (double)pb.eInfo[e], err);
      s += huber(st ? deltaStereo : deltaMono, c, &w);
    }
    return block_sum_d<BA_W>(s, red);
  };

  if (terminate()) {  // Optimizer.cc:1355-1356
    if (tid == 0) { pb.stats[0] = 0; pb.stats[1] = 0; }
    return;
  }
  double lambda = 0, ni = 2;
  int nBad = 0, its = 0, trials = 0;
  for (int iter = 0; iter < 10; ++iter) {
    if (terminate()) break;
    ++its;
    double currentChi = chi2All();
    const double iniChi = currentChi;
    // ---- buildSystem ----
    // (1) per map point: Hll, bl
    for (int m = tid; m < nMP; m += BA_T) {
      double Hl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
      const double* X = pb.pt + 3 * m;
      for (int k = pb.mpStart[m]; k < pb.mpStart[m + 1]; ++k) {
        const int e = pb.mpEdges[k];
        const SE3 T = load_se3(pb.pose + 7 * pb.eKF[e]);
        double xc[3], err[3], w, R[9], Jl[9];
        se3_map(T, X, xc);
        const float* o = pb.eObs + 3 * e;
        const bool st = !(o[2] < 0);
        const double info = (double)pb.eInfo[e];
        const double c = ba_edge_error(cam, pb.rig, st, xc, o, info, err);
        huber(st ? deltaStereo : deltaMono, c, &w);
        q_to_R(T.q, R);
        if (pb.rig) ba_edge_jac<true>(cam, pb.rig, st, xc, o, R, nullptr, Jl); else ba_edge_jac<false>(cam, pb.rig, st, xc, o, R, nullptr, Jl);   // (persistent mode: one kernel for both cameras)
        const double wo = w * info;
        for (int r = 0; r < 3; ++r) {
          double s = 0;
          _Pragma("unroll") for (int i = 0; i < 3; ++i) s += Jl[i * 3 + r] * (-info * err[i] * w);
          bl[r] += s;
          for (int cc = 0; cc < 3; ++cc) {
            double h = 0;
            _Pragma("unroll") for (int i = 0; i < 3; ++i) h += Jl[i * 3 + r] * wo * Jl[i * 3 + cc];
            Hl[r * 3 + cc] += h;
          }
        }
      }
      for (int k = 0; k < 9; ++k) pb.Hll[(size_t)m * 9 + k] = Hl[k];
      for (int k = 0; k < 3; ++k) pb.b[P + 3 * m + k] = bl[k];
    }
    // (2) per free keyframe (one wave each): Hpp, bp; per edge: Hpl
    for (int kf = wv; kf < nKF; kf += BA_W) {
      const int col = pb.kfCol[kf];
      if (col < 0) continue;
      const SE3 T = load_se3(pb.pose + 7 * kf);
      double R[9];
      q_to_R(T.q, R);
      double acc[27];
#pragma unroll
      for (int k = 0; k < 27; ++k) acc[k] = 0;
      for (int k = pb.kfStart[kf] + lane; k < pb.kfStart[kf + 1]; k += 64) {
        const int e = pb.kfEdges[k];
        double xc[3], err[3], w, Jp[18], Jl[9];
        se3_map(T, pb.pt + 3 * pb.eMP[e], xc);
        const float* o = pb.eObs + 3 * e;
        const bool st = !(o[2] < 0);
        const double info = (double)pb.eInfo[e];
        const double c = ba_edge_error(cam, pb.rig, st, xc, o, info, err);
        huber(st ? deltaStereo : deltaMono, c, &w);
        if (pb.rig) ba_edge_jac<true>(cam, pb.rig, st, xc, o, R, Jp, Jl); else ba_edge_jac<false>(cam, pb.rig, st, xc, o, R, Jp, Jl);
        const double wo = w * info;
        int q = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          double s = 0;
          _Pragma("unroll") for (int i = 0; i < 3; ++i) s += Jp[i * 6 + r] * (-info * err[i] * w);
          acc[21 + r] += s;
#pragma unroll
          for (int cc = r; cc < 6; ++cc) {
            double h = 0;
            _Pragma("unroll") for (int i = 0; i < 3; ++i) h += Jp[i * 6 + r] * wo * Jp[i * 6 + cc];
            acc[q++] += h;
          }
          for (int cc = 0; cc < 3; ++cc) {
            double h = 0;
            _Pragma("unroll") for (int i = 0; i < 3; ++i) h += Jp[i * 6 + r] * wo * Jl[i * 3 + cc];
            pb.Hpl[(size_t)e * 18 + r * 3 + cc] = h;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 27; ++k) acc[k] = wave_sum_d(acc[k]);
      if (lane == 0) {
        int q = 0;
        for (int r = 0; r < 6; ++r)
          for (int cc = r; cc < 6; ++cc) { pb.Hpp[(size_t)col * 36 + r * 6 + cc] = acc[q]; pb.Hpp[(size_t)col * 36 + cc * 6 + r] = acc[q]; ++q; }
        for (int r = 0; r < 6; ++r) pb.b[6 * col + r] = acc[21 + r];
      }
    }
    __syncthreads();
    if (iter == 0) {  // computeLambdaInit
      if (pb.userLambda > 0) lambda = pb.userLambda;
      else {
        double m = 0;
        for (int i = tid; i < pb.nFree * 6; i += BA_T) m = fmax(m, fabs(pb.Hpp[(size_t)(i / 6) * 36 + (i % 6) * 7]));
        for (int i = tid; i < nMP * 3; i += BA_T) m = fmax(m, fabs(pb.Hll[(size_t)(i / 3) * 9 + (i % 3) * 4]));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
        __syncthreads();
        if (lane == 0) red[wv] = m;
        __syncthreads();
        m = 0;
        for (int i = 0; i < BA_W; ++i) m = fmax(m, red[i]);
        lambda = 1e-5 * m;
      }
      ni = 2; nBad = 0;
    }
    double rho = 0;
    int qmax = 0;
    do {
      // push()
      for (int i = tid; i < nKF * 7; i += BA_T) pb.poseBk[i] = pb.pose[i];
      for (int i = tid; i < nMP * 3; i += BA_T) pb.ptBk[i] = pb.pt[i];
      // ---- BlockSolver::solve (Schur) with lambda on every diagonal (block_solver.hpp:354-480) ----
      // (a) per map point: Dinv = (Hll + lambda I)^-1
      for (int m = tid; m < nMP; m += BA_T) {
        double D[9], Di[9];
        for (int k = 0; k < 9; ++k) D[k] = pb.Hll[(size_t)m * 9 + k];
        D[0] += lambda; D[4] += lambda; D[8] += lambda;
        inv3(D, Di);
        for (int k = 0; k < 9; ++k) pb.Dinv[(size_t)m * 9 + k] = Di[k];
      }
      for (int i = tid; i < P * P; i += BA_T) Hs[i] = 0;
      __syncthreads();
      // (b) one wave per block pair (i1 <= i2): Hschur(i1,i2) = [Hpp + lambda I] - sum_l (Hpl_i1 Dinv_l) Hpl_i2^T,
      //     entries summed in a fixed order (deterministic), mirrored into the lower triangle
      for (int bp = wv; bp < pb.nPairs; bp += BA_W) {
        const int i1 = pb.pairBlock[bp] / pb.nFree, i2 = pb.pairBlock[bp] % pb.nFree;
        double acc[36];
#pragma unroll
        for (int k = 0; k < 36; ++k) acc[k] = 0;
        for (int k = pb.pairStart[bp] + lane; k < pb.pairStart[bp + 1]; k += 64) {
          const int2 en = pb.pairEntries[k];
          const double* B1 = pb.Hpl + (size_t)en.x * 18;
          const double* B2 = pb.Hpl + (size_t)en.y * 18;
          const double* Di = pb.Dinv + (size_t)pb.eMP[en.x] * 9;
          double BD[18];
#pragma unroll
          for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) BD[r * 3 + c] = B1[r * 3] * Di[c] + B1[r * 3 + 1] * Di[3 + c] + B1[r * 3 + 2] * Di[6 + c];
#pragma unroll
          for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) acc[r * 6 + c] += BD[r * 3] * B2[c * 3] + BD[r * 3 + 1] * B2[c * 3 + 1] + BD[r * 3 + 2] * B2[c * 3 + 2];
        }
#pragma unroll
        for (int k = 0; k < 36; ++k) acc[k] = wave_sum_d(acc[k]);
        if (lane < 36) {
          const int r = lane / 6, c = lane % 6;
          double a = 0;
#pragma unroll
          for (int k = 0; k < 36; ++k) if (k == lane) a = acc[k];
          double v = -a;
          if (i1 == i2) { v += pb.Hpp[(size_t)i1 * 36 + lane]; if (r == c) v += lambda; }
          Hs[(size_t)(6 * i1 + r) * P + 6 * i2 + c] = v;
          if (i1 != i2) Hs[(size_t)(6 * i2 + c) * P + 6 * i1 + r] = v;
        }
      }
      // (c) bschur = bp - sum Hpl Dinv bl, one wave per free keyframe over its CSR edge list
      for (int kf = wv; kf < nKF; kf += BA_W) {
        const int col = pb.kfCol[kf];
        if (col < 0) continue;
        double a6[6] = {0, 0, 0, 0, 0, 0};
        for (int k = pb.kfStart[kf] + lane; k < pb.kfStart[kf + 1]; k += 64) {
          const int e = pb.kfEdges[k];
          const int m = pb.eMP[e];
          const double* Di = pb.Dinv + (size_t)m * 9;
          const double* bl = pb.b + P + 3 * m;
          double db[3];
          for (int r = 0; r < 3; ++r) db[r] = Di[r * 3] * bl[0] + Di[r * 3 + 1] * bl[1] + Di[r * 3 + 2] * bl[2];
          const double* B1 = pb.Hpl + (size_t)e * 18;
          for (int r = 0; r < 6; ++r) a6[r] += B1[r * 3] * db[0] + B1[r * 3 + 1] * db[1] + B1[r * 3 + 2] * db[2];
        }
        for (int r = 0; r < 6; ++r) a6[r] = wave_sum_d(a6[r]);
        if (lane == 0) for (int r = 0; r < 6; ++r) pb.x[6 * col + r] = pb.b[6 * col + r] - a6[r];
      }
      __syncthreads();
      // (d) reduced system: right-looking LDL^T by the whole workgroup (LinearSolverEigen / SimplicialLDLT:
      //     fails only on a zero pivot), then the two triangular solves by wave 0
      if (tid == 0) sFlag = 1;
      __syncthreads();
      for (int j = 0; j < P; ++j) {
        const double d = Hs[(size_t)j * P + j];
        if (d == 0 || d != d) { if (tid == 0) sFlag = 0; break; }   // uniform: every thread reads the same d
        __syncthreads();
        // trailing update with the UNSCALED column: A_ik -= A_ij * A_kj / d  (i >= k > j), then scale column j
        const int nrem = P - j - 1;
        for (int t = tid; t < nrem * nrem; t += BA_T) {
          const int i = j + 1 + t / nrem, k = j + 1 + t % nrem;
          if (k <= i) Hs[(size_t)i * P + k] -= Hs[(size_t)i * P + j] * Hs[(size_t)k * P + j] / d;
        }
        __syncthreads();
        for (int i = j + 1 + tid; i < P; i += BA_T) Hs[(size_t)i * P + j] /= d;
      }
      __syncthreads();
      if (sFlag != 0 && wv == 0) {
        for (int j = 0; j < P; ++j) {           // forward: L y = b
          const double xj = pb.x[j];
          for (int i = j + 1 + lane; i < P; i += 64) pb.x[i] -= Hs[(size_t)i * P + j] * xj;
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
          __builtin_amdgcn_wave_barrier();
        }
        for (int i = lane; i < P; i += 64) pb.x[i] /= Hs[(size_t)i * P + i];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (int j = P - 1; j >= 0; --j) {      // backward: L^T x = y
          const double xj = pb.x[j];
          for (int i = lane; i < j; i += 64) pb.x[i] -= Hs[(size_t)j * P + i] * xj;
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
          __builtin_amdgcn_wave_barrier();
        }
      }
      __syncthreads();
      const bool ok2 = sFlag != 0;
      if (ok2) {
        // xl = Dinv * (bl - Hpl^T xp)
        for (int m = tid; m < nMP; m += BA_T) {
          double cl[3] = {pb.b[P + 3 * m], pb.b[P + 3 * m + 1], pb.b[P + 3 * m + 2]};
          for (int a = pb.mpStart[m]; a < pb.mpStart[m + 1]; ++a) {
            const int e = pb.mpEdges[a];
            const int i1 = pb.kfCol[pb.eKF[e]];
            if (i1 < 0) continue;
            const double* B = pb.Hpl + (size_t)e * 18;
            for (int c = 0; c < 3; ++c)
              for (int r = 0; r < 6; ++r) cl[c] -= B[r * 3 + c] * pb.x[6 * i1 + r];
          }
          const double* Di = pb.Dinv + (size_t)m * 9;
          for (int r = 0; r < 3; ++r) pb.x[P + 3 * m + r] = Di[r * 3] * cl[0] + Di[r * 3 + 1] * cl[1] + Di[r * 3 + 2] * cl[2];
        }
      } else {
        for (int i = tid; i < P + 3 * nMP; i += BA_T) pb.x[i] = 0;
      }
      __syncthreads();
      // update (oplus)
      for (int kf = tid; kf < nKF; kf += BA_T) {
        const int col = pb.kfCol[kf];
        if (col < 0) continue;
        double u[6];
        for (int r = 0; r < 6; ++r) u[r] = pb.x[6 * col + r];
        store_se3(pb.pose + 7 * kf, se3_mul(se3_exp(u), load_se3(pb.pose + 7 * kf)));
      }
      for (int i = tid; i < nMP * 3; i += BA_T) pb.pt[i] += pb.x[P + i];
      __syncthreads();
      double tempChi = chi2All();
      if (!ok2) tempChi = 1.7976931348623157e308;
      rho = currentChi - tempChi;
      double part = 0;
      for (int i = tid; i < P + 3 * nMP; i += BA_T) part += pb.x[i] * (lambda * pb.x[i] + pb.b[i]);
      double scale = block_sum_d<BA_W>(part, red) + 1e-3;
      rho /= scale;
      if (rho > 0 && isfinite(tempChi)) {
        double alpha = 1. - cube_rn(2 * rho - 1);
        alpha = fmin(alpha, 2. / 3.);
        lambda *= fmax(1. / 3., alpha);
        ni = 2;
        currentChi = tempChi;
      } else {
        lambda *= ni;
        ni *= 2;
        __syncthreads();
        for (int i = tid; i < nKF * 7; i += BA_T) pb.pose[i] = pb.poseBk[i];
        for (int i = tid; i < nMP * 3; i += BA_T) pb.pt[i] = pb.ptBk[i];
        __syncthreads();
      }
      ++qmax; ++trials;
    } while (rho < 0 && qmax < 10 && !terminate());
    if (qmax == 10 || rho == 0) break;
    if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
    if (nBad >= 3) break;
  }
  __syncthreads();
  // ---- post: chi2 / depth gates on the stored errors (state of the last evaluation), write-back as float ----
  for (int e = tid; e < nE; e += BA_T) {
    const float* o = pb.eObs + 3 * e;
    const bool st = !(o[2] < 0);
    double xc[3], err[3];
    se3_map(load_se3(pb.poseEval + 7 * pb.eKF[e]), pb.ptEval + 3 * pb.eMP[e], xc);
    const double c = ba_edge_error(cam, pb.rig, st, xc, o, (double)pb.eInfo[e], err);
    se3_map(load_se3(pb.pose + 7 * pb.eKF[e]), pb.pt + 3 * pb.eMP[e], xc);
    pb.erase[e] = (c > (st ? 7.815 : 5.991) || !ba_depth_positive(pb.rig, o, xc)) ? 1 : 0;
  }
  for (int kf = tid; kf < nKF; kf += BA_T)
    if (pb.kfCol[kf] >= 0) for (int k = 0; k < 7; ++k) pb.poseIO[7 * kf + k] = (float)pb.pose[7 * kf + k];
  for (int i = tid; i < nMP * 3; i += BA_T) pb.ptIO[i] = (float)pb.pt[i];
  if (tid == 0) { pb.stats[0] = its; pb.stats[1] = trials; }
}

// ---------------------------------------------------------------------------------------------------
// Grid mode: the same LM, one launch per phase over the whole chip; the accept/reject decision is taken on the
// host from three doubles read back once per trial (chi2, scale, ok).  Every reduction has a fixed order
// (block partials summed by one block; chunk partials summed per keyframe), so results are deterministic.
constexpr int GB = 256;

// LM state (grid mode, device-side control).  A phase kernel launched with gated = 1 returns at once when the solve has finished
// (launches are queued one trial ahead of the decisions) or, for the build kernels, when this trial re-solves the same system
// with a larger lambda (the previous trial was rejected).
enum { LM_ITER, LM_QMAX, LM_NBAD, LM_ITS, LM_TRIALS, LM_DONE, LM_NEEDBUILD, LM_REJECTED, LM_TICKET };
enum { LMD_CHI, LMD_LAMBDA, LMD_NI, LMD_INICHI };
__device__ __forceinline__ bool lm_skip(const BaDev& pb, int gated) { return gated && pb.lmi[LM_DONE] != 0; }
__device__ __forceinline__ bool lm_skip_build(const BaDev& pb, int gated) { return gated && (pb.lmi[LM_DONE] != 0 || pb.lmi[LM_NEEDBUILD] == 0); }
__device__ __forceinline__ bool lm_stop_requested(const BaDev& pb) {   // morb_ba_set_stop's flag and the caller's *pbStopFlag as the host loop forwards it
  return pb.stop && (__hip_atomic_load(pb.stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0 ||
                     __hip_atomic_load(pb.stop + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0);
}

// after the first chi2 (sum s): currentChi, and the state at the top of the first iteration.  One thread.
__device__ void lm_init(const BaDev& pb, double s) {
  const bool stop = lm_stop_requested(pb);
  pb.scal[0] = s;
  pb.lmd[LMD_CHI] = s; pb.lmd[LMD_LAMBDA] = 0; pb.lmd[LMD_NI] = 2; pb.lmd[LMD_INICHI] = s;
  pb.lmi[LM_ITER] = 0; pb.lmi[LM_QMAX] = 0; pb.lmi[LM_NBAD] = 0; pb.lmi[LM_ITS] = stop ? 0 : 1; pb.lmi[LM_TRIALS] = 0;
  pb.lmi[LM_DONE] = stop ? 1 : 0; pb.lmi[LM_NEEDBUILD] = 1; pb.lmi[LM_REJECTED] = 0;
  __hip_atomic_store(pb.lmHost + 2, stop ? 0 : 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(pb.lmHost + 3, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(pb.lmHost + 1, stop ? 1 : 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// after a trial's chi2 (s0) and linear-model gain (s1): rho, accept / reject, the lambda schedule, and whether another trial /
// iteration follows (optimization_algorithm_levenberg.cpp:99-169 with ORB-SLAM's stop rule).  One thread.
__device__ void lm_decide(const BaDev& pb, double s0, double s1) {
  pb.scal[0] = s0; pb.scal[1] = s1;
  double currentChi = pb.lmd[LMD_CHI], lambda = pb.lmd[LMD_LAMBDA], ni = pb.lmd[LMD_NI];
  const double iniChi = pb.lmd[LMD_INICHI];
  int iter = pb.lmi[LM_ITER], qmax = pb.lmi[LM_QMAX], nBad = pb.lmi[LM_NBAD], its = pb.lmi[LM_ITS];
  double tempChi = s0;
  if (pb.scal[2] == 0.0) tempChi = 1.7976931348623157e308;   // the linear solve failed
  const double rho = (currentChi - tempChi) / (s1 + 1e-3);
  const bool accept = rho > 0 && isfinite(tempChi);
  if (accept) {
    double alpha = 1. - cube_rn(2 * rho - 1);
    alpha = fmin(alpha, 2. / 3.);
    lambda *= fmax(1. / 3., alpha);
    ni = 2;
    currentChi = tempChi;
  } else {
    lambda *= ni;
    ni *= 2;
  }
  ++qmax;
  const int trials = pb.lmi[LM_TRIALS] + 1;
  const bool stop = lm_stop_requested(pb);
  int done = 0, needBuild = 0;
  if (!(rho < 0 && qmax < 10 && !stop)) {   // the trial loop ends (:139)
    bool fin = (qmax == 10 || rho == 0);
    if (!fin) { if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0; fin = nBad >= 3; }   // the stop rule of ORB-SLAM's g2o (:146-151)
    if (!fin) { ++iter; fin = iter >= 10 || stop; }
    if (fin) done = 1;
    else { ++its; qmax = 0; needBuild = 1; pb.lmd[LMD_INICHI] = currentChi; }
  }
  pb.lmd[LMD_CHI] = currentChi; pb.lmd[LMD_LAMBDA] = lambda; pb.lmd[LMD_NI] = ni;
  pb.lmi[LM_ITER] = iter; pb.lmi[LM_QMAX] = qmax; pb.lmi[LM_NBAD] = nBad; pb.lmi[LM_ITS] = its; pb.lmi[LM_TRIALS] = trials;
  pb.lmi[LM_DONE] = done; pb.lmi[LM_NEEDBUILD] = needBuild; pb.lmi[LM_REJECTED] = accept ? 0 : 1;
  __hip_atomic_store(pb.lmHost + 2, its, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(pb.lmHost + 3, trials, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(pb.lmHost + 1, done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(pb.lmHost + 0, trials, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // decided trials: the host queues trial k + 2 when it sees k
}
// In-launch hand-off of partial sums to the workgroup that draws the last ticket (guide, guideline 16): the payload is stored write-through
// at agent scope (sc1), the storing wave waits for its stores (s_waitcnt vmcnt(0)) and only then draws its ticket with a relaxed agent-scope
// add; the last arriver reads every handed-off word at agent scope (load_l2).  No __threadfence(): on this chip an agent-scope release is a
// write-back of the XCD's L2, and one per wave (k_g_build: 324 of them, beside the landmark half's stores) was ~8 of the kernel's 18 us.
__device__ __forceinline__ void store_l2(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wait_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ int draw_ticket(int* counter) { return __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double load_l2(const double* p) {   // another workgroup of this launch wrote it: read at agent scope
  return __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// mode 0: block partial sums only (host-side LM control).  mode 1 / 2 (device-side control): the last workgroup to finish adds the
// partials up in k_g_reduce's order and takes the LM decision of this trial (1) or sets up the first iteration (2).
__global__ __launch_bounds__(GB) void k_g_chi2(const BaDev* __restrict__ pbp, double* __restrict__ part, const double* __restrict__ part1, int mode) {
  __shared__ double red[4];
  __shared__ int isLast;
  const BaDev pb = *pbp;
  if (lm_skip(pb, mode == 1)) return;
  const int gid = blockIdx.x * GB + threadIdx.x;
  if (gid < pb.nKF * 7) pb.poseEval[gid] = pb.pose[gid];
  if (gid < pb.nMP * 3) pb.ptEval[gid] = pb.pt[gid];
  double s = 0;
  if (gid < pb.nE) {
    const SE3 T = load_se3(pb.pose + 7 * pb.eKF[gid]);
    double xc[3], err[3], w;
    se3_map(T, pb.pt + 3 * pb.eMP[gid], xc);
    const float* o = pb.eObs + 3 * gid;
    const bool st = !(o[2] < 0);
    const double c = ba_edge_error(pb.cam, pb.rig, st, xc, o, (double)pb.eInfo[gid], err);
    s = huber(st ? (double)(float)sqrt(7.815) : (double)(float)sqrt(5.991), c, &w);
  }
  s = block_sum_d<4>(s, red);
  if (threadIdx.x == 0) store_l2(part + blockIdx.x, s);
  if (mode == 0) return;
  if (threadIdx.x == 0) {
    wait_stores();
    isLast = draw_ticket(&pb.lmi[LM_TICKET]) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!isLast) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (every handed-off word is read with load_l2)
  const int n = gridDim.x;
  double s0 = 0, s1 = 0;
  for (int i = threadIdx.x; i < n; i += GB) { s0 += load_l2(part + i); if (mode == 1) s1 += load_l2(part1 + i); }
  s0 = block_sum_d<4>(s0, red);
  s1 = block_sum_d<4>(s1, red);
  if (threadIdx.x != 0) return;
  pb.lmi[LM_TICKET] = 0;
  if (mode == 1) lm_decide(pb, s0, s1); else lm_init(pb, s0);
}
// The landmark blocks Hll / bl of map point m (block_solver.hpp:354-480 reads them): EIGHT lanes per point, one edge each and chunk by chunk
// (a point has 5 - 8 observations here; a thread per point walked them one after the other: 20 of k_g_build's 23 us).  Each lane leaves its
// edge's twelve contributions in the wave's LDS slice and the group's first lane adds them up IN EDGE ORDER — the sums are bit for bit those
// of the serial walk.  Lanes of one wave only: no workgroup barrier.  -> max |diag Hll| of the point (first lane of the group; 0 elsewhere)
constexpr int MP_LANES = 8;
template <bool RIG>
__device__ __forceinline__ double build_mp_point(const BaDev& pb, int m, int sub, double* __restrict__ slot /* [MP_LANES][12] of the group */) {
  const double deltaMono = (double)(float)sqrt(5.991), deltaStereo = (double)(float)sqrt(7.815);
  double Hl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
  const bool live = m < pb.nMP;
  const double* X = pb.pt + 3 * (live ? m : 0);
  const int k0 = live ? pb.mpStart[m] : 0, k1 = live ? pb.mpStart[m + 1] : 0;
  for (int kb = k0; kb < k1; kb += MP_LANES) {
    const int k = kb + sub;
    double c12[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) c12[q] = 0;
    if (k < k1) {
      const int e = pb.mpEdges[k];
      const SE3 T = load_se3(pb.pose + 7 * pb.eKF[e]);
      double xc[3], err[3], w, R[9], Jl[9];
      se3_map(T, X, xc);
      const float* o = pb.eObs + 3 * e;
      const bool st = !(o[2] < 0);
      const double info = (double)pb.eInfo[e];
      const double c = ba_edge_error(pb.cam, pb.rig, st, xc, o, info, err);
      huber(st ? deltaStereo : deltaMono, c, &w);
      q_to_R(T.q, R);
      ba_edge_jac<RIG>(pb.cam, pb.rig, st, xc, o, R, nullptr, Jl);
      const double wo = w * info;   // (mono edges: third Jacobian row and err[2] are zero, so the 3-row form is exact)
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double sacc = 0;
        _Pragma("unroll") for (int i = 0; i < 3; ++i) sacc += Jl[i * 3 + r] * (-info * err[i] * w);
        c12[9 + r] = sacc;
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
          double h = 0;
          _Pragma("unroll") for (int i = 0; i < 3; ++i) h += Jl[i * 3 + r] * wo * Jl[i * 3 + cc];
          c12[r * 3 + cc] = h;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) slot[sub * 12 + q] = c12[q];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (sub == 0) {
      const int cnt = k1 - kb < MP_LANES ? k1 - kb : MP_LANES;
      for (int j = 0; j < cnt; ++j) {
#pragma unroll
        for (int q = 0; q < 9; ++q) Hl[q] += slot[j * 12 + q];
#pragma unroll
        for (int q = 0; q < 3; ++q) bl[q] += slot[j * 12 + 9 + q];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   // (the slice is rewritten by the next chunk)
  }
  if (!live || sub != 0) return 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) pb.Hll[(size_t)m * 9 + k] = Hl[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) pb.b[pb.P + 3 * m + k] = bl[k];
  return fmax(fmax(fabs(Hl[0]), fabs(Hl[4])), fabs(Hl[8]));
}
template <bool RIG>
__device__ __forceinline__ void build_kf_chunk(const BaDev& pb, int c, int lane) {
  const int kf = pb.chunkKF[c];
  const double deltaMono = (double)(float)sqrt(5.991), deltaStereo = (double)(float)sqrt(7.815);
  const SE3 T = load_se3(pb.pose + 7 * kf);
  double R[9];
  q_to_R(T.q, R);
  double acc[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) acc[k] = 0;
  const int k = pb.chunkStart[c] + lane;
  if (k < pb.chunkEnd[c]) {
    const int e = pb.kfEdges[k];
    double xc[3], err[3], w, Jp[18], Jl[9];
    se3_map(T, pb.pt + 3 * pb.eMP[e], xc);
    const float* o = pb.eObs + 3 * e;
    const bool st = !(o[2] < 0);
    const double info = (double)pb.eInfo[e];
    const double ch = ba_edge_error(pb.cam, pb.rig, st, xc, o, info, err);
    huber(st ? deltaStereo : deltaMono, ch, &w);
    ba_edge_jac<RIG>(pb.cam, pb.rig, st, xc, o, R, Jp, Jl);
    const double wo = w * info;   // (mono edges: third Jacobian row and err[2] are zero, so the 3-row form is exact)
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double sacc = 0;
      _Pragma("unroll") for (int i = 0; i < 3; ++i) sacc += Jp[i * 6 + r] * (-info * err[i] * w);
      acc[21 + r] = sacc;
#pragma unroll
      for (int cc = r; cc < 6; ++cc) {
        double h = 0;
        _Pragma("unroll") for (int i = 0; i < 3; ++i) h += Jp[i * 6 + r] * wo * Jp[i * 6 + cc];
        acc[q++] = h;
      }
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) {
        double h = 0;
        _Pragma("unroll") for (int i = 0; i < 3; ++i) h += Jp[i * 6 + r] * wo * Jl[i * 3 + cc];
        pb.Hpl[(size_t)e * 18 + r * 3 + cc] = h;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 27; ++q) acc[q] = wave_sum_d(acc[q]);
  if (lane < 27) {
    double v = 0;
#pragma unroll
    for (int q = 0; q < 27; ++q) if (q == lane) v = acc[q];
    store_l2(pb.kfPart + (size_t)c * 27 + lane, v);
  }
}
// buildSystem in ONE launch (device-side LM control): workgroups [0, kfBlocks) take the keyframe chunks, the rest the map points;
// the last chunk of a keyframe to deliver its partial blocks adds them up in chunk order (k_g_kf_reduce's sum, whoever runs it).
// Two launches on two streams cost more in cross-stream events (~25 us per trial) than running side by side saved.
template <bool RIG>
__global__ __launch_bounds__(GB) void k_g_build(const BaDev* __restrict__ pbp, int kfBlocks) {
  const BaDev pb = *pbp;
  if (lm_skip_build(pb, 1)) return;
  // first iteration: the largest diagonal entry of the system for computeLambdaInit (:186-194) — a max is order-independent, so an
  // atomic on the bit pattern of the non-negative double keeps the result deterministic
  const bool first = pb.lmi[LM_TRIALS] == 0;
  unsigned long long* maxDiag = reinterpret_cast<unsigned long long*>(pb.scal + 3);
  if ((int)blockIdx.x >= kfBlocks) {
    __shared__ double sMp[GB * 12];
    const int g = threadIdx.x / MP_LANES, sub = threadIdx.x % MP_LANES;
    const int m = (blockIdx.x - kfBlocks) * (GB / MP_LANES) + g;
    double dm = build_mp_point<RIG>(pb, m, sub, sMp + (size_t)g * MP_LANES * 12);
    if (first) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) dm = fmax(dm, __shfl_xor(dm, off, 64));
      if ((threadIdx.x & 63) == 0) atomicMax(maxDiag, __builtin_bit_cast(unsigned long long, dm));
    }
    return;
  }
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= pb.nChunks) return;
  build_kf_chunk<RIG>(pb, c, lane);
  const int kf = pb.chunkKF[c];
  int last = 0;
  wait_stores();   // (the wave's partial sums have left for memory)
  if (lane == 0) {
    const int nc = pb.kfChunkStart[kf + 1] - pb.kfChunkStart[kf];
    last = draw_ticket(&pb.kfTicket[kf]) == nc - 1;
    if (last) pb.kfTicket[kf] = 0;
  }
  if (!__builtin_amdgcn_readfirstlane(last)) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (every handed-off word is read with load_l2)
  const int col = pb.kfCol[kf];
  if (lane >= 27) return;
  double s = 0;
  for (int cc = pb.kfChunkStart[kf]; cc < pb.kfChunkStart[kf + 1]; ++cc) s += load_l2(pb.kfPart + (size_t)cc * 27 + lane);
  if (lane < 21) {
    int r = 0, q = lane;
    while (q >= 6 - r) { q -= 6 - r; ++r; }
    const int c2 = r + q;
    pb.Hpp[(size_t)col * 36 + r * 6 + c2] = s;
    pb.Hpp[(size_t)col * 36 + c2 * 6 + r] = s;
    if (first && r == c2) atomicMax(maxDiag, __builtin_bit_cast(unsigned long long, fabs(s)));
  } else {
    pb.b[6 * col + (lane - 21)] = s;
  }
}
// Hpl of (keyframe column i, landmark m) as the MFMA operands need it: a fisheye rig may observe a landmark with both cameras
// of one keyframe, i.e. through two edges — the first of them (lowest edge index) carries the sum, the others nothing.
__device__ __forceinline__ bool pair_block(const BaDev& pb, int e, int i, int m, double* __restrict__ B) {
  for (int q = 0; q < 18; ++q) B[q] = pb.Hpl[(size_t)e * 18 + q];
  if (!pb.dupPairs) return true;
  for (int k = pb.mpStart[m]; k < pb.mpStart[m + 1]; ++k) {
    const int e2 = pb.mpEdges[k];
    if (e2 == e || pb.kfCol[pb.eKF[e2]] != i) continue;
    if (e2 < e) return false;
    for (int q = 0; q < 18; ++q) B[q] += pb.Hpl[(size_t)e2 * 18 + q];
  }
  return true;
}
// Start of a trial.  gated (device-side LM control): lambda comes from the LM state; a rejected previous trial is undone here
// (pose / point backup restored instead of taken), and after an accepted one the operand W is packed too (k_g_pack_w's work).
__global__ __launch_bounds__(GB) void k_g_dinv_push(const BaDev* __restrict__ pbp, double lambda, double* __restrict__ Hs, int valuSchur, int gated) {
  const BaDev pb = *pbp;
  if (lm_skip(pb, gated)) return;
  bool restore = false, packW = false;
  const int gid = blockIdx.x * GB + threadIdx.x;
  if (gated) {
    lambda = pb.lmd[LMD_LAMBDA]; restore = pb.lmi[LM_REJECTED] != 0; packW = pb.lmi[LM_NEEDBUILD] != 0;
    if (pb.lmi[LM_TRIALS] == 0) {   // first trial: computeLambdaInit (:186-194) from the build's max diagonal; later kernels read it from the state
      lambda = pb.userLambda > 0 ? pb.userLambda : 1e-5 * pb.scal[3];
      if (gid == 0) pb.lmd[LMD_LAMBDA] = lambda;
    }
  }
  if (restore) {
    if (gid < pb.nKF * 7) pb.pose[gid] = pb.poseBk[gid];
    if (gid < pb.nMP * 3) pb.pt[gid] = pb.ptBk[gid];
  } else {
    if (gid < pb.nKF * 7) pb.poseBk[gid] = pb.pose[gid];
    if (gid < pb.nMP * 3) pb.ptBk[gid] = pb.pt[gid];
  }
  if (valuSchur && gid < pb.P * pb.P) Hs[gid] = 0;
  if (gid < pb.nMP) {
    double D[9], Di[9];
    for (int k = 0; k < 9; ++k) D[k] = pb.Hll[(size_t)gid * 9 + k];
    D[0] += lambda; D[4] += lambda; D[8] += lambda;
    inv3(D, Di);
    for (int k = 0; k < 9; ++k) pb.Dinv[(size_t)gid * 9 + k] = Di[k];
  }
  if (!valuSchur && gid < pb.nE) {
    // the MFMA operand WD = Hpl (Hll + lambda I)^-1 of this observation (rows 3 m + c, columns 6 i + r); the inverse is
    // recomputed per observation so that the pack needs no second launch behind the per-point loop above
    const int i = pb.kfCol[pb.eKF[gid]];
    const int m = pb.eMP[gid];
    double B1[18];
    if (i >= 0 && pair_block(pb, gid, i, m, B1)) {
      double D[9], Di[9];
      for (int k = 0; k < 9; ++k) D[k] = pb.Hll[(size_t)m * 9 + k];
      D[0] += lambda; D[4] += lambda; D[8] += lambda;
      inv3(D, Di);
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          pb.sWD[(size_t)(3 * m + c) * pb.sMp + 6 * i + r] = B1[r * 3] * Di[c] + B1[r * 3 + 1] * Di[3 + c] + B1[r * 3 + 2] * Di[6 + c];
          if (packW) pb.sW[(size_t)(3 * m + c) * pb.sMp + 6 * i + r] = B1[r * 3 + c];
        }
    }
  }
  if (packW && gid < pb.nMP * 3) pb.sW[(size_t)gid * pb.sMp + pb.P] = pb.b[pb.P + gid];
}
// reduced system from the partial products: Hs = Hpp + lambda I - C (C symmetric: the upper blocks serve both triangles),
// x[0:P] = b_p - C[:, P]
__global__ __launch_bounds__(GB) void k_g_schur_finish(const BaDev* __restrict__ pbp, double lambda, double* __restrict__ Hs, int gated) {
  const BaDev pb = *pbp;
  if (lm_skip(pb, gated)) return;
  if (gated) lambda = pb.lmd[LMD_LAMBDA];
  const int t = blockIdx.x * GB + threadIdx.x, gid = t >> 2, q = t & 3, P = pb.P;   // four lanes per element (schur_sum4)
  const bool mat = gid < P * P, rhs = !mat && gid < P * P + P;
  int r = 0, c = P;
  if (mat) { r = gid / P; c = gid - r * P; } else if (rhs) r = gid - P * P;
  const int i = r < c ? r : c, j = r < c ? c : r;
  const double cs = morbschur::schur_sum4(pb.sPart, pb.sBlkIndex, pb.sNb, pb.sNblk, pb.sNsplit, (mat || rhs) ? i : 0, (mat || rhs) ? j : 0, q);
  if (q != 0) return;
  if (mat) {
    double v = -cs;
    if (r / 6 == c / 6) { v += pb.Hpp[(size_t)(r / 6) * 36 + (r % 6) * 6 + (c % 6)]; if (r == c) v += lambda; }
    Hs[gid] = v;
  } else if (rhs) {
    pb.x[r] = pb.b[r] - cs;
  }
}
// the reduced camera system beyond 163 unknowns (28 free keyframes and more: the reference takes every covisible keyframe,
// Optimizer.cc:1058-1070): the matrix stays in global memory, one 16-column panel at a time in LDS (dense_ldlt.h: ldlt_solve_global);
// HsG is overwritten by the factors (k_g_schur_finish rebuilds it for every trial); x = Hs^-1 x in place
__global__ __launch_bounds__(morbdense::GT) void k_g_ldlt_global(const BaDev* __restrict__ pbp, double* __restrict__ HsG, double* __restrict__ pnlG,
                                                                 int panelInLds, int gated) {
  extern __shared__ double sLd[];   // dblk | y | (the panel copies when they fit)
  __shared__ int sOk;
  const BaDev pb = *pbp;
  if (lm_skip(pb, gated)) return;
  double* pnl = panelInLds ? sLd + morbdense::global_lds_doubles(pb.P) : pnlG;
  const bool ok = morbdense::ldlt_solve_global<false>(HsG, pb.x, pb.x, pb.P, pnl, sLd, &sOk);
  if (threadIdx.x == 0) pb.scal[2] = ok ? 1.0 : 0.0;
}
// the reduced camera system with its lower triangle resident in LDS (dense_ldlt.h); x = Hs^-1 x in place
__global__ __launch_bounds__(morbdense::LT) void k_g_ldlt_lds(const BaDev* __restrict__ pbp, const double* __restrict__ HsG, int gated) {
  extern __shared__ double sLd[];
  __shared__ int sOk;
  const BaDev pb = *pbp;
  if (lm_skip(pb, gated)) return;
  const bool ok = morbdense::ldlt_solve<false>(HsG, pb.x, pb.x, pb.P, sLd, &sOk);
  if (threadIdx.x == 0) pb.scal[2] = ok ? 1.0 : 0.0;
}
// The same step with the landmark part read from the MFMA operand W (dense rows [3 nMP][Mp], column P = b_l): 16 lanes per point,
// lane q takes columns q, q + 16, ... of the point's three rows (coalesced 128-byte reads, all in flight at once) and the row sums are
// DPP reductions in a fixed order — round 2's first form walked the point's edges one dependent load chain after the other (21 us).
__global__ __launch_bounds__(GB) void k_g_backsub_update_w(const BaDev* __restrict__ pbp, double* __restrict__ part) {
  __shared__ double red[4];
  const BaDev pb = *pbp;
  if (lm_skip(pb, 1)) return;
  const double lambda = pb.lmd[LMD_LAMBDA];
  const int gid = blockIdx.x * GB + threadIdx.x, m = gid >> 4, q = gid & 15;
  const int P = pb.P;
  const bool ok = pb.scal[2] != 0.0;
  double sc = 0;
  {
    const bool live = m < pb.nMP;
    const size_t row = (size_t)3 * (live ? m : 0) * pb.sMp;
    double a0 = 0, a1 = 0, a2 = 0;
    for (int j = q; j < P; j += 16) {
      const double xj = pb.x[j];
      a0 += pb.sW[row + j] * xj; a1 += pb.sW[row + pb.sMp + j] * xj; a2 += pb.sW[row + 2 * (size_t)pb.sMp + j] * xj;
    }
    a0 = morbwave::row_sum_f64(a0); a1 = morbwave::row_sum_f64(a1); a2 = morbwave::row_sum_f64(a2);
    if (live && q < 3) {
      double xl = 0;
      if (ok) {
        const double cl[3] = {pb.sW[row + P] - a0, pb.sW[row + pb.sMp + P] - a1, pb.sW[row + 2 * (size_t)pb.sMp + P] - a2};
        const double* Di = pb.Dinv + (size_t)m * 9;
        xl = Di[q * 3] * cl[0] + Di[q * 3 + 1] * cl[1] + Di[q * 3 + 2] * cl[2];
      }
      pb.x[P + 3 * m + q] = xl;
      pb.pt[3 * m + q] += xl;
      sc += xl * (lambda * xl + pb.b[P + 3 * m + q]);
    }
  }
  if (gid < pb.nKF) {
    const int col = pb.kfCol[gid];
    if (col >= 0) {
      double u[6];
      for (int r = 0; r < 6; ++r) { u[r] = ok ? pb.x[6 * col + r] : 0.0; sc += u[r] * (lambda * u[r] + pb.b[6 * col + r]); }
      store_se3(pb.pose + 7 * gid, se3_mul(se3_exp(u), load_se3(pb.pose + 7 * gid)));
    }
  }
  sc = block_sum_d<4>(sc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = sc;
}
__global__ __launch_bounds__(GB) void k_g_finish(const BaDev* __restrict__ pbp, int its, int trials) {
  const BaDev pb = *pbp;
  const double *pose = pb.pose, *pt = pb.pt;
  if (its < 0) {   // device-side LM control keeps the counters; a rejected last trial is undone by reading its backup
    its = pb.lmi[LM_ITS]; trials = pb.lmi[LM_TRIALS];
    if (pb.lmi[LM_REJECTED]) { pose = pb.poseBk; pt = pb.ptBk; }
  }
  const int gid = blockIdx.x * GB + threadIdx.x;
  if (gid < pb.nE) {
    const int e = gid;
    const float* o = pb.eObs + 3 * e;
    const bool st = !(o[2] < 0);
    double xc[3], err[3];
    se3_map(load_se3(pb.poseEval + 7 * pb.eKF[e]), pb.ptEval + 3 * pb.eMP[e], xc);
    const double c = ba_edge_error(pb.cam, pb.rig, st, xc, o, (double)pb.eInfo[e], err);
    se3_map(load_se3(pose + 7 * pb.eKF[e]), pt + 3 * pb.eMP[e], xc);
    pb.erase[e] = (c > (st ? 7.815 : 5.991) || !ba_depth_positive(pb.rig, o, xc)) ? 1 : 0;
  }
  if (gid < pb.nKF && pb.kfCol[gid] >= 0) for (int k = 0; k < 7; ++k) pb.poseIO[7 * gid + k] = (float)pose[7 * gid + k];
  if (gid < pb.nMP * 3) pb.ptIO[gid] = (float)pt[gid];
  if (gid == 0) { pb.stats[0] = its; pb.stats[1] = trials; }
}

// ---- device-side LM control (optimization_algorithm_levenberg.cpp:61-169 as morb_ba_solve's host loop used to run it) ----
__global__ void k_ba_reset(BaDev pb, const float* __restrict__ pose0, const float* __restrict__ pt0) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < pb.nKF) {
    const SE3 s = se3_from_float(pose0 + 7 * i);
    store_se3(pb.pose + 7 * i, s);
    for (int k = 0; k < 7; ++k) pb.poseIO[7 * i + k] = pose0[7 * i + k];
  }
  if (i < pb.nMP * 3) pb.pt[i] = (double)pt0[i];
  if (i == 0) { pb.lmi[LM_TICKET] = 0; pb.scal[3] = 0; }
}

// =====================================================================================================
// The welding bundle adjustment of map merging: Optimizer::LocalBundleAdjustment(KeyFrame* pMainKF, vector<KeyFrame*> vpAdjustKF,
// vector<KeyFrame*> vpFixedKF, bool* pbStopFlag) (reference src/Optimizer.cc:3430-3851, called at src/LoopClosing.cc:1652).  Grid mode only,
// LM control on the device.  Two rounds in ONE queue of launches: optimize(5) with Huber kernels (deltas (float)sqrt(5.99) / (float)sqrt(7.815),
// :3547-3548), then every edge with chi2() > 5.991 / 7.815 or a non-positive depth goes to level 1, every edge loses its kernel, and
// initializeOptimization(0); optimize(10) runs over the level-0 edges (:3662-3698).  The graph, the workspace and the phases that do not look at an
// edge's error (k_g_dinv_push, k_schur_mfma, k_g_schur_finish, k_g_ldlt_*, k_g_backsub_update_w) are LocalBundleAdjustment's; the three that do —
// chi2, build, finish — are restated here with the round state and the level mask.
//   * A level-1 edge contributes exact zeros wherever a level-0 edge contributes its terms: chi2, Hll / bl, the chunk sums of Hpp / bp, and its
//     Hpl block is stored as zeros, so the Schur operands W / WD (packed from Hpl) and the back-substitution (which reads W) carry zeros too.
//     Sums keep LocalBundleAdjustment's fixed order; x + 0 is x, so the blocks are those of the graph without the edge.
//   * A vertex whose edges are all on level 1 (g2o drops it from the active set) keeps H = 0, b = 0: its damped block is lambda I, its right-hand
//     side 0, its update exactly 0 (0 / lambda; nothing divides by the empty block itself), and |diag| = 0 leaves computeLambdaInit's maximum alone.
//   * chiEdge[e] is chi2() of the edge as g2o holds it: written by every evaluation of an active edge (computeActiveErrors), i.e. after a rejected
//     last trial the rejected trial's value, and for a level-1 edge the value it had when it was classified (it is never active again, :3705-3739).
//   * The decision that ends round 1 (mlm_decide) raises RS_TRANSITION and closes the gate of the phase kernels (LM_DONE) without telling the host:
//     the next slot of the queue is then empty except for its k_mg_chi2, which classifies, undoes a rejected last trial, evaluates the level-0
//     edges without kernels and starts round 2's LM (iteration 0: lambda = tau max diag of the NEW system, ni = 2, nBad = 0,
//     optimization_algorithm_levenberg.cpp:93-96).  The host only counts slots and watches `done`.
struct MergeDev {
  BaDev ba;                 // first member: the phase kernels shared with LocalBundleAdjustment take this descriptor's address
  uint8_t* level;           // [nE] 1 = the edge is on level 1 (excluded from round 2)
  double* chiEdge;          // [nE]
  int* rs;                  // [16] RS_*: the round state, beside ba.lmi
  int* stats6;              // [6]
  double deltaMono, deltaStereo;   // Huber deltas of this optimiser
};
enum { RS_ROUND, RS_CAP, RS_ROBUST, RS_TRANSITION, RS_SLOTS, RS_ITS1, RS_TRIALS1, RS_NLEVEL1 };

// the state at the top of a round's first iteration, after its first chi2 (sum s).  One thread.
__device__ void mlm_init(const MergeDev& md, double s, int round) {
  const BaDev& pb = md.ba;
  const bool stop = lm_stop_requested(pb);
  pb.scal[0] = s; pb.scal[3] = 0;   // (round 2's computeLambdaInit: the maximum starts again)
  pb.lmd[LMD_CHI] = s; pb.lmd[LMD_LAMBDA] = 0; pb.lmd[LMD_NI] = 2; pb.lmd[LMD_INICHI] = s;
  pb.lmi[LM_ITER] = 0; pb.lmi[LM_QMAX] = 0; pb.lmi[LM_NBAD] = 0; pb.lmi[LM_ITS] = stop ? 0 : 1; pb.lmi[LM_TRIALS] = 0;
  pb.lmi[LM_DONE] = stop ? 1 : 0; pb.lmi[LM_NEEDBUILD] = 1; pb.lmi[LM_REJECTED] = 0;
  md.rs[RS_ROUND] = round; md.rs[RS_CAP] = round ? 10 : 5; md.rs[RS_ROBUST] = round ? 0 : 1; md.rs[RS_TRANSITION] = 0;
  const int slots = round ? md.rs[RS_SLOTS] + 1 : 0;   // (the hand-over took a slot of the queue)
  md.rs[RS_SLOTS] = slots;
  __hip_atomic_store(pb.lmHost + 1, stop ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(pb.lmHost + 0, slots, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// lm_decide with the round's iteration cap, and the end of round 1 handing over to round 2 (Optimizer.cc:3654-3698).  One thread.
__device__ void mlm_decide(const MergeDev& md, double s0, double s1) {
  const BaDev& pb = md.ba;
  pb.scal[0] = s0; pb.scal[1] = s1;
  double currentChi = pb.lmd[LMD_CHI], lambda = pb.lmd[LMD_LAMBDA], ni = pb.lmd[LMD_NI];
  const double iniChi = pb.lmd[LMD_INICHI];
  int iter = pb.lmi[LM_ITER], qmax = pb.lmi[LM_QMAX], nBad = pb.lmi[LM_NBAD], its = pb.lmi[LM_ITS];
  const int cap = md.rs[RS_CAP], round = md.rs[RS_ROUND];
  double tempChi = s0;
  if (pb.scal[2] == 0.0) tempChi = 1.7976931348623157e308;   // the linear solve failed
  const double rho = (currentChi - tempChi) / (s1 + 1e-3);
  const bool accept = rho > 0 && isfinite(tempChi);
  if (accept) {
    double alpha = 1. - cube_rn(2 * rho - 1);
    alpha = fmin(alpha, 2. / 3.);
    lambda *= fmax(1. / 3., alpha);
    ni = 2;
    currentChi = tempChi;
  } else {
    lambda *= ni;
    ni *= 2;
  }
  ++qmax;
  const int trials = pb.lmi[LM_TRIALS] + 1;
  const bool stop = lm_stop_requested(pb);
  int gate = 0, done = 0, needBuild = 0;
  if (!(rho < 0 && qmax < 10 && !stop)) {   // the trial loop ends (:139)
    bool fin = (qmax == 10 || rho == 0);
    if (!fin) { if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0; fin = nBad >= 3; }
    if (!fin) { ++iter; fin = iter >= cap || stop; }
    if (fin) {
      gate = 1;
      if (round == 0 && !stop) { md.rs[RS_ITS1] = its; md.rs[RS_TRIALS1] = trials; md.rs[RS_TRANSITION] = 1; }   // *pbStopFlag clear at :3658: round 2 follows
      else done = 1;
    } else { ++its; qmax = 0; needBuild = 1; pb.lmd[LMD_INICHI] = currentChi; }
  }
  pb.lmd[LMD_CHI] = currentChi; pb.lmd[LMD_LAMBDA] = lambda; pb.lmd[LMD_NI] = ni;
  pb.lmi[LM_ITER] = iter; pb.lmi[LM_QMAX] = qmax; pb.lmi[LM_NBAD] = nBad; pb.lmi[LM_ITS] = its; pb.lmi[LM_TRIALS] = trials;
  pb.lmi[LM_DONE] = gate; pb.lmi[LM_NEEDBUILD] = needBuild; pb.lmi[LM_REJECTED] = accept ? 0 : 1;
  const int slots = md.rs[RS_SLOTS] + 1;
  md.rs[RS_SLOTS] = slots;
  __hip_atomic_store(pb.lmHost + 1, done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(pb.lmHost + 0, slots, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // decided slots: the host queues slot k + 2 when it sees k
}
__global__ void k_mg_reset(MergeDev md) {
  if (threadIdx.x < 16) md.rs[threadIdx.x] = threadIdx.x == RS_CAP ? 5 : threadIdx.x == RS_ROBUST ? 1 : 0;
  if (threadIdx.x < 6) md.stats6[threadIdx.x] = 0;
}
// mode 2: the first chi2 of round 1.  mode 1: a trial's chi2 and its LM decision — or, in the slot behind round 1's last decision, the hand-over:
// every edge is classified on chiEdge and on its depth at the estimate the round left (the backup when its last trial was rejected, which is
// restored here), and the level-0 edges' plain chi2 there opens round 2.
__global__ __launch_bounds__(GB) void k_mg_chi2(const MergeDev* __restrict__ mdp, double* __restrict__ part, const double* __restrict__ part1, int mode) {
  __shared__ double red[4];
  __shared__ int isLast;
  const MergeDev md = *mdp;
  const BaDev& pb = md.ba;
  const bool trans = mode == 1 && md.rs[RS_TRANSITION] != 0;
  if (!trans && lm_skip(pb, mode == 1)) return;
  const bool robust = !trans && md.rs[RS_ROBUST] != 0;
  const bool undo = trans && pb.lmi[LM_REJECTED] != 0;
  const double *pose = undo ? pb.poseBk : pb.pose, *pt = undo ? pb.ptBk : pb.pt;
  const int gid = blockIdx.x * GB + threadIdx.x;
  double s = 0;
  bool bad = false;
  if (gid < pb.nE) {
    const float* o = pb.eObs + 3 * gid;
    const bool st = !(o[2] < 0);
    double xc[3], err[3], w;
    se3_map(load_se3(pose + 7 * pb.eKF[gid]), pt + 3 * pb.eMP[gid], xc);
    if (trans) {
      bad = md.chiEdge[gid] > (st ? 7.815 : 5.991) || !ba_depth_positive(pb.rig, o, xc);   // :3671 / :3684
      md.level[gid] = bad ? 1 : 0;
    }
    if (trans ? !bad : md.level[gid] == 0) {
      const double c = ba_edge_error(pb.cam, pb.rig, st, xc, o, (double)pb.eInfo[gid], err);
      md.chiEdge[gid] = c;
      s = robust ? huber(st ? md.deltaStereo : md.deltaMono, c, &w) : c;
    }
  }
  if (trans) {
    const int nb = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0 && nb) atomicAdd(&md.rs[RS_NLEVEL1], nb);   // (an integer count: any order gives the same sum; read by k_mg_finish)
    if (undo) {   // (the readers of this launch take the backup itself)
      if (gid < pb.nKF * 7) pb.pose[gid] = pb.poseBk[gid];
      if (gid < pb.nMP * 3) pb.pt[gid] = pb.ptBk[gid];
    }
  }
  s = block_sum_d<4>(s, red);
  if (threadIdx.x == 0) {
    store_l2(part + blockIdx.x, s);
    wait_stores();
    isLast = draw_ticket(&pb.lmi[LM_TICKET]) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!isLast) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (every handed-off word is read with load_l2)
  const int n = gridDim.x;
  const bool decide = mode == 1 && !trans;
  double s0 = 0, s1 = 0;
  for (int i = threadIdx.x; i < n; i += GB) { s0 += load_l2(part + i); if (decide) s1 += load_l2(part1 + i); }
  s0 = block_sum_d<4>(s0, red);
  s1 = block_sum_d<4>(s1, red);
  if (threadIdx.x != 0) return;
  pb.lmi[LM_TICKET] = 0;
  if (decide) mlm_decide(md, s0, s1); else mlm_init(md, s0, trans ? 1 : 0);
}
// build_mp_point / build_kf_chunk / k_g_build with the level mask and the round's kernels
template <bool RIG>
__device__ __forceinline__ double mg_build_mp_point(const MergeDev& md, bool robust, int m, int sub, double* __restrict__ slot) {
  const BaDev& pb = md.ba;
  double Hl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
  const bool live = m < pb.nMP;
  const double* X = pb.pt + 3 * (live ? m : 0);
  const int k0 = live ? pb.mpStart[m] : 0, k1 = live ? pb.mpStart[m + 1] : 0;
  for (int kb = k0; kb < k1; kb += MP_LANES) {
    const int k = kb + sub;
    double c12[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) c12[q] = 0;
    const int e = k < k1 ? pb.mpEdges[k] : 0;
    if (k < k1 && md.level[e] == 0) {
      const SE3 T = load_se3(pb.pose + 7 * pb.eKF[e]);
      double xc[3], err[3], w = 1.0, R[9], Jl[9];
      se3_map(T, X, xc);
      const float* o = pb.eObs + 3 * e;
      const bool st = !(o[2] < 0);
      const double info = (double)pb.eInfo[e];
      const double c = ba_edge_error(pb.cam, pb.rig, st, xc, o, info, err);
      if (robust) huber(st ? md.deltaStereo : md.deltaMono, c, &w);
      q_to_R(T.q, R);
      ba_edge_jac<RIG>(pb.cam, pb.rig, st, xc, o, R, nullptr, Jl);
      const double wo = w * info;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double sacc = 0;
        _Pragma("unroll") for (int i = 0; i < 3; ++i) sacc += Jl[i * 3 + r] * (-info * err[i] * w);
        c12[9 + r] = sacc;
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
          double h = 0;
          _Pragma("unroll") for (int i = 0; i < 3; ++i) h += Jl[i * 3 + r] * wo * Jl[i * 3 + cc];
          c12[r * 3 + cc] = h;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) slot[sub * 12 + q] = c12[q];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (sub == 0) {
      const int cnt = k1 - kb < MP_LANES ? k1 - kb : MP_LANES;
      for (int j = 0; j < cnt; ++j) {
#pragma unroll
        for (int q = 0; q < 9; ++q) Hl[q] += slot[j * 12 + q];
#pragma unroll
        for (int q = 0; q < 3; ++q) bl[q] += slot[j * 12 + 9 + q];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   // (the slice is rewritten by the next chunk)
  }
  if (!live || sub != 0) return 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) pb.Hll[(size_t)m * 9 + k] = Hl[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) pb.b[pb.P + 3 * m + k] = bl[k];
  return fmax(fmax(fabs(Hl[0]), fabs(Hl[4])), fabs(Hl[8]));
}
template <bool RIG>
__device__ __forceinline__ void mg_build_kf_chunk(const MergeDev& md, bool robust, int c, int lane) {
  const BaDev& pb = md.ba;
  const int kf = pb.chunkKF[c];
  const SE3 T = load_se3(pb.pose + 7 * kf);
  double R[9];
  q_to_R(T.q, R);
  double acc[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) acc[k] = 0;
  const int k = pb.chunkStart[c] + lane;
  if (k < pb.chunkEnd[c]) {
    const int e = pb.kfEdges[k];
    if (md.level[e] != 0) {
#pragma unroll
      for (int q = 0; q < 18; ++q) pb.Hpl[(size_t)e * 18 + q] = 0.0;
    } else {
      double xc[3], err[3], w = 1.0, Jp[18], Jl[9];
      se3_map(T, pb.pt + 3 * pb.eMP[e], xc);
      const float* o = pb.eObs + 3 * e;
      const bool st = !(o[2] < 0);
      const double info = (double)pb.eInfo[e];
      const double ch = ba_edge_error(pb.cam, pb.rig, st, xc, o, info, err);
      if (robust) huber(st ? md.deltaStereo : md.deltaMono, ch, &w);
      ba_edge_jac<RIG>(pb.cam, pb.rig, st, xc, o, R, Jp, Jl);
      const double wo = w * info;
      int q = 0;
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        double sacc = 0;
        _Pragma("unroll") for (int i = 0; i < 3; ++i) sacc += Jp[i * 6 + r] * (-info * err[i] * w);
        acc[21 + r] = sacc;
#pragma unroll
        for (int cc = r; cc < 6; ++cc) {
          double h = 0;
          _Pragma("unroll") for (int i = 0; i < 3; ++i) h += Jp[i * 6 + r] * wo * Jp[i * 6 + cc];
          acc[q++] = h;
        }
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
          double h = 0;
          _Pragma("unroll") for (int i = 0; i < 3; ++i) h += Jp[i * 6 + r] * wo * Jl[i * 3 + cc];
          pb.Hpl[(size_t)e * 18 + r * 3 + cc] = h;
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 27; ++q) acc[q] = wave_sum_d(acc[q]);
  if (lane < 27) {
    double v = 0;
#pragma unroll
    for (int q = 0; q < 27; ++q) if (q == lane) v = acc[q];
    store_l2(pb.kfPart + (size_t)c * 27 + lane, v);
  }
}
template <bool RIG>
__global__ __launch_bounds__(GB) void k_mg_build(const MergeDev* __restrict__ mdp, int kfBlocks) {
  const MergeDev md = *mdp;
  const BaDev& pb = md.ba;
  if (lm_skip_build(pb, 1)) return;
  const bool robust = md.rs[RS_ROBUST] != 0;
  const bool first = pb.lmi[LM_TRIALS] == 0;   // (of this round)
  unsigned long long* maxDiag = reinterpret_cast<unsigned long long*>(pb.scal + 3);
  if ((int)blockIdx.x >= kfBlocks) {
    __shared__ double sMp[GB * 12];
    const int g = threadIdx.x / MP_LANES, sub = threadIdx.x % MP_LANES;
    const int m = (blockIdx.x - kfBlocks) * (GB / MP_LANES) + g;
    double dm = mg_build_mp_point<RIG>(md, robust, m, sub, sMp + (size_t)g * MP_LANES * 12);
    if (first) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) dm = fmax(dm, __shfl_xor(dm, off, 64));
      if ((threadIdx.x & 63) == 0) atomicMax(maxDiag, __builtin_bit_cast(unsigned long long, dm));
    }
    return;
  }
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= pb.nChunks) return;
  mg_build_kf_chunk<RIG>(md, robust, c, lane);
  const int kf = pb.chunkKF[c];
  int last = 0;
  wait_stores();
  if (lane == 0) {
    const int nc = pb.kfChunkStart[kf + 1] - pb.kfChunkStart[kf];
    last = draw_ticket(&pb.kfTicket[kf]) == nc - 1;
    if (last) pb.kfTicket[kf] = 0;
  }
  if (!__builtin_amdgcn_readfirstlane(last)) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int col = pb.kfCol[kf];
  if (lane >= 27) return;
  double s = 0;
  for (int cc = pb.kfChunkStart[kf]; cc < pb.kfChunkStart[kf + 1]; ++cc) s += load_l2(pb.kfPart + (size_t)cc * 27 + lane);
  if (lane < 21) {
    int r = 0, q = lane;
    while (q >= 6 - r) { q -= 6 - r; ++r; }
    const int c2 = r + q;
    pb.Hpp[(size_t)col * 36 + r * 6 + c2] = s;
    pb.Hpp[(size_t)col * 36 + c2 * 6 + r] = s;
    if (first && r == c2) atomicMax(maxDiag, __builtin_bit_cast(unsigned long long, fabs(s)));
  } else {
    pb.b[6 * col + (lane - 21)] = s;
  }
}
// the erase rule (:3705-3739) on chiEdge and the depth at the final estimate, the write-back as float, stats6
__global__ __launch_bounds__(GB) void k_mg_finish(const MergeDev* __restrict__ mdp) {
  const MergeDev md = *mdp;
  const BaDev& pb = md.ba;
  const bool undo = pb.lmi[LM_REJECTED] != 0;   // a rejected last trial is undone by reading its backup
  const double *pose = undo ? pb.poseBk : pb.pose, *pt = undo ? pb.ptBk : pb.pt;
  const int gid = blockIdx.x * GB + threadIdx.x;
  if (gid < pb.nE) {
    const float* o = pb.eObs + 3 * gid;
    const bool st = !(o[2] < 0);
    double xc[3];
    se3_map(load_se3(pose + 7 * pb.eKF[gid]), pt + 3 * pb.eMP[gid], xc);
    pb.erase[gid] = (md.chiEdge[gid] > (st ? 7.815 : 5.991) || !ba_depth_positive(pb.rig, o, xc)) ? 1 : 0;
  }
  if (gid < pb.nKF && pb.kfCol[gid] >= 0) for (int k = 0; k < 7; ++k) pb.poseIO[7 * gid + k] = (float)pose[7 * gid + k];
  if (gid < pb.nMP * 3) pb.ptIO[gid] = (float)pt[gid];
  if (gid == 0) {
    const int round = md.rs[RS_ROUND];
    md.stats6[0] = round ? md.rs[RS_ITS1] : pb.lmi[LM_ITS]; md.stats6[1] = round ? md.rs[RS_TRIALS1] : pb.lmi[LM_TRIALS];
    md.stats6[2] = round ? pb.lmi[LM_ITS] : 0; md.stats6[3] = round ? pb.lmi[LM_TRIALS] : 0;
    md.stats6[4] = md.rs[RS_NLEVEL1]; md.stats6[5] = round + 1;
  }
}

}  // namespace

// =====================================================================================================
struct morb_ba_problem {
  morb_optimizer* opt = nullptr;
  BaDev h;                 // host copy of the device descriptor
  BaDev* d_desc = nullptr;
  float *d_pose0 = nullptr, *d_pt0 = nullptr;
  // a persistent problem (three-step API) owns its device block and pinned words; a one-shot problem borrows them from the optimizer handle
  morb::DeviceArray<> mem;
  morb::PinnedArray<int> words;
  int* h_stop = nullptr;   // [16] pinned, device-mapped host words: [0] abort flag (morb_ba_set_stop writes it without any HIP call, kernels poll it), [1] forwarded *pbStopFlag, [4..7] LM state mirror
  const volatile unsigned char* userStop = nullptr;   // the caller's *pbStopFlag (one-shot entry points), polled by the host LM loop
  int useLds = 1;
  size_t ldsBytes = 0;
  size_t denseLds = 0;     // LDS bytes of the triangle-resident solver (0: the system is too large for it)
  int mode = 0;            // 0 = grid (one launch per LM phase, host-side accept/reject), 1 = one persistent workgroup
  morb::Event solved;            // recorded behind the last morb_ba_solve on whatever stream it ran on: morb_ba_results waits for the EVENT — not for
                                 // the device, and not through the caller's stream handle, which the caller may have destroyed since
  int redBlocks = 0;
  morbschur::Plan schur;
  size_t nPairEntries = 0;   // (e1, e2) observation pairs of the sparse block-pair Schur form (flop accounting only)
  double* d_ldws = nullptr;  // panel copies of the global-memory LDL^T when they do not fit LDS (dense_ldlt.h: global_panel_doubles)
  size_t globalLds = 0;      // dynamic LDS of k_g_ldlt_global
  int panelInLds = 1;
};

// ---- the host side of a grid-mode solve that LocalBA and the welding BA share ----
// the launches of a slot between its build and its chi2: landmark inverses, Schur complement on the matrix cores, LDL^T, back-substitution
static void ba_launch_solve_phases(const morb_ba_problem* p, hipStream_t st) {
  const BaDev& h = p->h; const BaDev* d = p->d_desc; const int rb = p->redBlocks;
  hipLaunchKernelGGL(k_g_dinv_push, dim3(rb > div_up(h.P * h.P, GB) ? rb : div_up(h.P * h.P, GB)), dim3(GB), 0, st, d, 0.0, h.HsG, 0, 1);
  hipLaunchKernelGGL(morbschur::k_schur_mfma, dim3(p->schur.nblk, p->schur.nsplit), dim3(64), 0, st, (const double*)h.sWD,
                     (const double*)h.sW, p->schur.Mp, p->schur.ksteps, p->schur.stepsPerSplit, h.sBlocks, h.sPart, (const int*)(h.lmi + LM_DONE));
  hipLaunchKernelGGL(k_g_schur_finish, dim3(div_up(4 * (h.P * h.P + h.P), GB)), dim3(GB), 0, st, d, 0.0, h.HsG, 1);
  if (p->denseLds) hipLaunchKernelGGL(k_g_ldlt_lds, dim3(1), dim3(morbdense::LT), p->denseLds, st, d, (const double*)h.HsG, 1);
  else hipLaunchKernelGGL(k_g_ldlt_global, dim3(1), dim3(morbdense::GT), p->globalLds, st, d, h.HsG, p->d_ldws, p->panelInLds, 1);
  hipLaunchKernelGGL(k_g_backsub_update_w, dim3(rb), dim3(GB), 0, st, d, h.redPart + rb);
}

// A solve on st behind its reset kernels, through the queue of ba_host.h (lm_slot_queue): clears the forwarded stop flag and the LM state
// mirror (morb_ba_set_stop's word stays), lets launchSlot(slot) queue up to maxSlots slots, forwarding the caller's *pbStopFlag to the word
// the decision kernels poll before the first launch and at every look, then lets launchFinish() queue the adjuster's last kernel.
template <class LaunchSlot, class LaunchFinish>
static int ba_queue_solve(morb_ba_problem* p, hipStream_t st, int maxSlots, const char* who, LaunchSlot&& launchSlot, LaunchFinish&& launchFinish) {
  auto forwardStop = [&]() { if (p->userStop && *p->userStop) __atomic_store_n(p->h_stop + 1, 1, __ATOMIC_RELEASE); };
  reset_lm_words(p->h_stop + 4, 4, p->h_stop + 1);   // the mirror is h_stop[4 .. 7]: [4] decided, [5] done, [6] iterations, [7] trials; [1] the forwarded stop flag
  forwardStop();
  const int q = lm_slot_queue(maxSlots, p->h_stop + 4, p->h_stop + 5, [&](int slot) { launchSlot(slot); MORB_HIP_CHECK(hipGetLastError()); return MORB_OK; },
                              [&]() { return stream_look(st, who); }, forwardStop);
  if (q < 0) return MORB_ERR_HIP;
  launchFinish();
  MORB_HIP_CHECK(hipGetLastError());
  // slot limit reached without a `done`: decisions of this solve may still be on their way — let them land before the next solve resets
  // the mirror words (the usual exit has seen `done`, after which no kernel writes them)
  if (!q) MORB_HIP_CHECK(hipStreamSynchronize(st));
  return MORB_OK;
}

// the read-back of the poses, the points and the erase flags, queued on st (null: not wanted); the caller adds its own and synchronises
static hipError_t ba_queue_results(const morb_ba_problem* p, hipStream_t st, float* kfPose, float* mpPos, uint8_t* eraseFlag) {
  hipError_t e = kfPose ? hipMemcpyAsync(kfPose, p->h.poseIO, sizeof(float) * 7 * p->h.nKF, hipMemcpyDeviceToHost, st) : hipSuccess;
  if (e == hipSuccess && mpPos) e = hipMemcpyAsync(mpPos, p->h.ptIO, sizeof(float) * 3 * p->h.nMP, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && eraseFlag) e = hipMemcpyAsync(eraseFlag, p->h.erase, p->h.nE, hipMemcpyDeviceToHost, st);
  return e;
}

extern "C" {

// what every entry point refuses before anything else: a missing array, an empty graph, an edge that names no keyframe or map point
static int ba_check_graph(const morb_optimizer* o, int nKF, const float* kfPose, const uint8_t* kfFixed, int nMP, const float* mpPos, int nE,
                          const int* eKF, const int* eMP, const float* eObs, const float* eInvSigma2) {
  MORB_REQUIRE(o && kfPose && kfFixed && mpPos && eKF && eMP && eObs && eInvSigma2, MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nKF > 0 && nMP > 0 && nE > 0, MORB_ERR_INVALID, "empty problem");
  for (int e = 0; e < nE; ++e) MORB_REQUIRE(eKF[e] >= 0 && eKF[e] < nKF && eMP[e] >= 0 && eMP[e] < nMP, MORB_ERR_INVALID, "edge index out of range");
  return MORB_OK;
}

// the two-float observations of a fisheye entry point in the three-float form of the graph: the edge kind travels in the third slot,
// -2 = EdgeSE3ProjectXYZ with the left KB8 camera, -3 = EdgeSE3ProjectXYZToBody (right KB8 camera behind mTrl; eRight == null: no such edge)
static std::vector<float> fisheye_obs3(int nE, const float* eObs2, const uint8_t* eRight) {
  std::vector<float> obs3((size_t)nE * 3);
  for (int e = 0; e < nE; ++e) { obs3[3 * e] = eObs2[2 * e]; obs3[3 * e + 1] = eObs2[2 * e + 1]; obs3[3 * e + 2] = eRight && eRight[e] ? -3.0f : -2.0f; }
  return obs3;
}

// morb_ba_problem_create, with the fisheye rig of morb_ba_problem_create_fisheye (nullptr: pinhole).  arena: the problem of a one-shot
// entry point, carved from the handle's `work` / `stage` / `lmWords` for the duration of that call (it owns no memory of its own)
static int ba_problem_create(morb_optimizer* o, morb_ba_problem** out, int nKF, const float* kfPose, const uint8_t* kfFixed,
                             int nMP, const float* mpPos, int nE, const int* eKF, const int* eMP, const float* eObs,
                             const float* eInvSigma2, float fx, float fy, float cx, float cy, float bf,
                             int lambdaInit100, const Rig* rig, bool arena, MergeDev* merge = nullptr) {
  MORB_REQUIRE(out, MORB_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (const int rc = ba_check_graph(o, nKF, kfPose, kfFixed, nMP, mpPos, nE, eKF, eMP, eObs, eInvSigma2)) return rc;
  MORB_HIP_CHECK(hipSetDevice(o->device));
  std::unique_ptr<morb_ba_problem> p(new morb_ba_problem());
  p->opt = o;
  BaDev& h = p->h;
  memset(&h, 0, sizeof h);
  h.nKF = nKF; h.nMP = nMP; h.nE = nE;
  std::vector<int> kfCol(nKF, -1);
  // free keyframes that actually carry an edge get a column (initializeOptimization drops isolated vertices)
  std::vector<char> used(nKF, 0);
  for (int e = 0; e < nE; ++e) used[eKF[e]] = 1;
  int nFree = 0;
  for (int i = 0; i < nKF; ++i) if (!kfFixed[i] && used[i]) kfCol[i] = nFree++;
  h.nFree = nFree; h.P = 6 * nFree;
  // CSR lists in edge-id order
  std::vector<int> mpStart, kfStart, mpEdges, kfEdges;
  csr_by_key(eMP, nE, nMP, mpStart, mpEdges);
  csr_by_key(eKF, nE, nKF, kfStart, kfEdges);
  h.dupPairs = 0;
  for (int m = 0; m < nMP && !h.dupPairs; ++m)
    for (int a = mpStart[m]; a < mpStart[m + 1] && !h.dupPairs; ++a)
      for (int b2 = a + 1; b2 < mpStart[m + 1]; ++b2)
        if (eKF[mpEdges[a]] == eKF[mpEdges[b2]]) { h.dupPairs = 1; break; }
  // block pairs of the reduced camera system and, per pair, the (observation, observation) entries that feed it: operands of the
  // persistent-workgroup mode.  The one-shot entry points always solve in grid
  // mode on the matrix cores, which only needs the number of entries (flop accounting): they skip the lists (0.3 ms of host work, 0.6 MB).
  std::vector<int> pairBlock, pairStart;
  std::vector<int2> pairEntries;
  const bool wantPairs = !arena;
  size_t nPairEntriesCount = 0;
  if (!wantPairs) {
    for (int m = 0; m < nMP; ++m) {
      size_t nf = 0;
      for (int a = mpStart[m]; a < mpStart[m + 1]; ++a) nf += kfCol[eKF[mpEdges[a]]] >= 0 ? 1 : 0;
      nPairEntriesCount += nf * (nf + 1) / 2;   // (pairs with column(e1) <= column(e2), as the lists would hold them; approximate for duplicate columns)
    }
    pairBlock.push_back(0); pairStart.assign(2, 0); pairEntries.assign(1, make_int2(0, 0));
  } else {
    const int nb = std::max(nFree, 1) * std::max(nFree, 1);
    std::vector<int> cnt(nb + 1, 0);
    auto forPairs = [&](auto&& fn) {
      for (int m = 0; m < nMP; ++m)
        for (int a = mpStart[m]; a < mpStart[m + 1]; ++a) {
          const int ea = mpEdges[a], ca = kfCol[eKF[ea]];
          if (ca < 0) continue;
          for (int b2 = mpStart[m]; b2 < mpStart[m + 1]; ++b2) {
            const int eb = mpEdges[b2], cb = kfCol[eKF[eb]];
            if (cb < 0 || cb < ca) continue;
            fn(ca * nFree + cb, ea, eb);
          }
        }
    };
    forPairs([&](int key, int, int) { cnt[key + 1]++; });
    std::vector<int> slot(nb, -1);
    int total = 0;
    for (int k = 0; k < nb; ++k) {
      if (cnt[k + 1] > 0) { slot[k] = (int)pairBlock.size(); pairBlock.push_back(k); pairStart.push_back(total); total += cnt[k + 1]; }
    }
    pairStart.push_back(total);
    pairEntries.resize(std::max(total, 1));
    std::vector<int> fill(pairStart.begin(), pairStart.end());
    forPairs([&](int key, int ea, int eb) { pairEntries[fill[slot[key]]++] = make_int2(ea, eb); });
  }
  h.nPairs = wantPairs ? (int)pairBlock.size() : 0;
  std::vector<int> chunkKF, chunkStart, chunkEnd, kfChunkStart;
  chunks_of(kfStart, kfCol.data(), 64, chunkKF, chunkStart, chunkEnd, &kfChunkStart);
  h.nChunks = (int)chunkKF.size();
  const morbschur::Plan sp = p->schur = morbschur::make_plan(h.P + 1, 3 * nMP);
  std::vector<int2> blocks; std::vector<int> blkIndex;
  schur_block_lists(sp.nb, blocks, blkIndex);
  bool fail = false;
  // Memory: every array is carved from ONE device block — uploads first, gathered in a host staging buffer and sent in ONE copy, device-only
  // arrays behind them — because ~45 hipMalloc / hipFree pairs and ~25 synchronous copies were 3.5 ms of a 4.7 ms call.  A dry run of the carve
  // sizes the block (ba_host.h).  The one-shot entry points (arena mode) take the block, the pinned staging buffer and the pinned words from the
  // optimizer handle; a persistent problem (three-step API) owns its block and words.
  ArenaCarver A;
  hipStream_t cst = o->stream;
  auto carve = [&]() {
  h.kfCol = (const int*)A.take(kfCol.data(), sizeof(int) * nKF);
  h.eKF = (const int*)A.take(eKF, sizeof(int) * nE);
  h.eMP = (const int*)A.take(eMP, sizeof(int) * nE);
  h.eObs = (const float*)A.take(eObs, sizeof(float) * 3 * nE);
  h.eInfo = (const float*)A.take(eInvSigma2, sizeof(float) * nE);
  h.mpStart = (const int*)A.take(mpStart.data(), sizeof(int) * (nMP + 1));
  h.mpEdges = (const int*)A.take(mpEdges.data(), sizeof(int) * nE);
  h.kfStart = (const int*)A.take(kfStart.data(), sizeof(int) * (nKF + 1));
  h.kfEdges = (const int*)A.take(kfEdges.data(), sizeof(int) * nE);
  h.pairBlock = (const int*)A.take(pairBlock.data(), sizeof(int) * std::max<size_t>(pairBlock.size(), 1));
  h.pairStart = (const int*)A.take(pairStart.data(), sizeof(int) * pairStart.size());
  h.pairEntries = (const int2*)A.take(pairEntries.data(), sizeof(int2) * pairEntries.size());
  p->nPairEntries = wantPairs ? pairEntries.size() : nPairEntriesCount;
  h.chunkKF = (const int*)A.take(chunkKF.data(), sizeof(int) * std::max<size_t>(chunkKF.size(), 1));
  h.chunkStart = (const int*)A.take(chunkStart.data(), sizeof(int) * std::max<size_t>(chunkStart.size(), 1));
  h.chunkEnd = (const int*)A.take(chunkEnd.data(), sizeof(int) * std::max<size_t>(chunkEnd.size(), 1));
  h.kfChunkStart = (const int*)A.take(kfChunkStart.data(), sizeof(int) * (nKF + 1));
  h.kfPart = (double*)A.take(nullptr, sizeof(double) * 27 * std::max<size_t>(chunkKF.size(), 1));
  p->d_ldws = (double*)A.take(nullptr, sizeof(double) * morbdense::global_panel_doubles(std::max(h.P, 1)));
  p->redBlocks = div_up(std::max(std::max(nE, nMP * 16), std::max(nKF * 7, 1)), GB);   // (16 lanes per point in k_g_backsub_update_w)
  h.redPart = (double*)A.take(nullptr, sizeof(double) * 2 * p->redBlocks);
  h.scal = (double*)A.take(nullptr, sizeof(double) * 8);
  h.sW = (double*)A.take(nullptr, sizeof(double) * sp.wElems());
  h.sWD = (double*)A.take(nullptr, sizeof(double) * sp.wElems());
  h.sPart = (double*)A.take(nullptr, sizeof(double) * sp.partElems());
  h.sBlocks = (const int2*)A.take(blocks.data(), sizeof(int2) * blocks.size());
  h.sBlkIndex = (const int*)A.take(blkIndex.data(), sizeof(int) * blkIndex.size());
  h.sMp = sp.Mp; h.sNb = sp.nb; h.sNblk = sp.nblk; h.sNsplit = sp.nsplit;
  const size_t nx = (size_t)h.P + 3 * (size_t)nMP;
  h.pose = (double*)A.take(nullptr, sizeof(double) * 7 * nKF);
  h.poseBk = (double*)A.take(nullptr, sizeof(double) * 7 * nKF);
  h.poseEval = (double*)A.take(nullptr, sizeof(double) * 7 * nKF);
  h.pt = (double*)A.take(nullptr, sizeof(double) * 3 * nMP);
  h.ptBk = (double*)A.take(nullptr, sizeof(double) * 3 * nMP);
  h.ptEval = (double*)A.take(nullptr, sizeof(double) * 3 * nMP);
  h.Hpp = (double*)A.take(nullptr, sizeof(double) * 36 * std::max(nFree, 1));
  h.Hll = (double*)A.take(nullptr, sizeof(double) * 9 * nMP);
  h.Dinv = (double*)A.take(nullptr, sizeof(double) * 9 * nMP);
  h.Hpl = (double*)A.take(nullptr, sizeof(double) * 18 * nE);
  h.b = (double*)A.take(nullptr, sizeof(double) * nx);
  h.x = (double*)A.take(nullptr, sizeof(double) * nx);
  h.HsG = (double*)A.take(nullptr, sizeof(double) * std::max<size_t>((size_t)h.P * h.P, 1));
  h.poseIO = (float*)A.take(nullptr, sizeof(float) * 7 * nKF);
  h.ptIO = (float*)A.take(nullptr, sizeof(float) * 3 * nMP);
  h.erase = (uint8_t*)A.take(nullptr, nE);
  h.stats = (int*)A.take(nullptr, sizeof(int) * 2);
  h.lmd = (double*)A.take(nullptr, sizeof(double) * 4);
  h.kfTicket = (int*)A.take(nullptr, sizeof(int) * std::max(nKF, 1));
  h.lmi = (int*)A.take(nullptr, sizeof(int) * 16);
  h.cam = Cam{fx, fy, cx, cy, bf};
  h.rig = rig ? (const Rig*)A.take(rig, sizeof(Rig)) : nullptr;
  h.userLambda = lambdaInit100 ? 100.0 : 0.0;
  p->d_pose0 = (float*)A.take(kfPose, sizeof(float) * 7 * nKF);
  p->d_pt0 = (float*)A.take(mpPos, sizeof(float) * 3 * nMP);
  if (merge) {   // the welding BA's descriptor: this one, then the level mask, the edges' chi2 and the round state
    merge->level = (uint8_t*)A.take(nullptr, nE);
    merge->chiEdge = (double*)A.take(nullptr, sizeof(double) * nE);
    merge->rs = (int*)A.take(nullptr, sizeof(int) * 16);
    merge->stats6 = (int*)A.take(nullptr, sizeof(int) * 6);
    merge->ba = h;
    p->d_desc = (BaDev*)A.take(merge, sizeof(MergeDev));
  } else {
    p->d_desc = (BaDev*)A.take(&h, sizeof(BaDev));
  }
  };   // carve
  carve();   // (dry: sizes)
  const size_t upCap = A.uploadBytes(), devCap = A.deviceBytes();
  char *aBase = nullptr, *stage = nullptr;
  std::vector<char> hostStage;   // a persistent problem's staging: pageable, the upload is waited for below
  if (arena) {
    if (grow(o->work, upCap + devCap, &aBase) != MORB_OK || grow(o->stage, upCap, &stage) != MORB_OK) fail = true;
  } else {
    if (p->mem.alloc(upCap + devCap) != hipSuccess) fail = true;
    hostStage.resize(upCap);
    aBase = (char*)p->mem.get(); stage = hostStage.data();
  }
  if (!fail) {   // mapped host words: [0] morb_ba_set_stop, [1] the caller's *pbStopFlag as the host loop forwards it, [4..7] the LM state mirror
    int *hw = nullptr, *dv = nullptr;
    if (arena) { if (morb_optimizer_lm_words(o, &hw, &dv) != MORB_OK) fail = true; }
    else if (p->words.alloc(sizeof(int) * 16, hipHostMallocMapped) != hipSuccess) fail = true;
    else { hw = p->words; dv = p->words.dev(); }
    if (hw) { memset(hw, 0, sizeof(int) * 16); p->h_stop = hw; h.stop = dv; h.lmHost = dv + 4; }
  }
  if (!fail) {
    A.bind(aBase, stage);
    carve();   // (the descriptor it stages last holds the pointers it has just assigned, and the words above)
    if (!A.ok() || hipMemsetAsync(h.sW, 0, sizeof(double) * sp.wElems(), cst) != hipSuccess ||
        hipMemsetAsync(h.sWD, 0, sizeof(double) * sp.wElems(), cst) != hipSuccess ||
        hipMemsetAsync(h.kfTicket, 0, sizeof(int) * std::max(nKF, 1), cst) != hipSuccess) fail = true;
    if (!fail && merge && hipMemsetAsync(merge->level, 0, nE, cst) != hipSuccess) fail = true;
    if (!fail && hipMemcpyAsync(aBase, stage, upCap, hipMemcpyHostToDevice, cst) != hipSuccess) fail = true;   // the one upload
    // a persistent problem is complete when create returns (like the synchronous copies it was once made with): it may be solved on any stream
    if (!fail && !arena && hipStreamSynchronize(cst) != hipSuccess) fail = true;
  }
  p->ldsBytes = sizeof(double) * (size_t)h.P * (h.P + 1);
  p->useLds = (p->ldsBytes <= morbdense::PERSISTENT_HS_LIMIT && h.P <= 192) ? 1 : 0;
  if (!p->useLds) p->ldsBytes = 0;
  p->denseLds = sizeof(double) * morbdense::lds_doubles(h.P);
  if (p->denseLds > morbdense::LDS_SOLVER_LIMIT || h.P < 1) p->denseLds = 0;   // larger systems: the global-memory solver
  if (!fail && p->denseLds && hipFuncSetAttribute(reinterpret_cast<const void*>(k_g_ldlt_lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)morbdense::LDS_SOLVER_LIMIT) != hipSuccess) fail = true;
  p->globalLds = sizeof(double) * (morbdense::global_lds_doubles(std::max(h.P, 1)) + morbdense::global_panel_doubles(std::max(h.P, 1)));
  p->panelInLds = p->globalLds <= morbdense::GLOBAL_SOLVER_LIMIT ? 1 : 0;
  if (!p->panelInLds) p->globalLds = sizeof(double) * morbdense::global_lds_doubles(std::max(h.P, 1));
  if (!fail && !p->denseLds && (p->globalLds > morbdense::GLOBAL_SOLVER_LIMIT ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(k_g_ldlt_global), hipFuncAttributeMaxDynamicSharedMemorySize, (int)morbdense::GLOBAL_SOLVER_LIMIT) != hipSuccess)) fail = true;
  if (!fail && p->useLds && hipFuncSetAttribute(reinterpret_cast<const void*>(k_local_ba), hipFuncAttributeMaxDynamicSharedMemorySize, (int)morbdense::PERSISTENT_HS_LIMIT) != hipSuccess)
    fail = true;
  if (fail) {
    set_error("device allocation/copy failed while creating the BA problem");
    return MORB_ERR_HIP;
  }
  *out = p.release();
  return MORB_OK;
}

int morb_ba_problem_create(morb_optimizer* o, morb_ba_problem** out, int nKF, const float* kfPose, const uint8_t* kfFixed,
                           int nMP, const float* mpPos, int nE, const int* eKF, const int* eMP, const float* eObs,
                           const float* eInvSigma2, float fx, float fy, float cx, float cy, float bf,
                           int lambdaInit100) {
  return ba_problem_create(o, out, nKF, kfPose, kfFixed, nMP, mpPos, nE, eKF, eMP, eObs, eInvSigma2, fx, fy, cx, cy, bf, lambdaInit100, nullptr, false);
}

void morb_ba_problem_destroy(morb_ba_problem* p) {
  if (!p) return;
  (void)hipSetDevice(p->opt->device);
  (void)hipStreamSynchronize(p->opt->stream);
  if (p->solved) (void)hipEventSynchronize(p->solved);
  delete p;
}

static int ba_problem_create_fisheye(morb_optimizer* o, morb_ba_problem** out, int nKF, const float* kfPose, const uint8_t* kfFixed,
                                     int nMP, const float* mpPos, int nE, const int* eKF, const int* eMP, const float* eObs2,
                                     const uint8_t* eRight, const float* eInvSigma2, const float* camL8, const float* camR8,
                                     const float* Trl7, int lambdaInit100, bool arena) {
  MORB_REQUIRE(out && eObs2 && eRight && camL8 && camR8 && Trl7, MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nE > 0, MORB_ERR_INVALID, "empty problem");
  const std::vector<float> obs3 = fisheye_obs3(nE, eObs2, eRight);
  const Rig rig = make_rig(camL8, camR8, Trl7);
  return ba_problem_create(o, out, nKF, kfPose, kfFixed, nMP, mpPos, nE, eKF, eMP, obs3.data(), eInvSigma2, 0.f, 0.f, 0.f, 0.f, 0.f,
                           lambdaInit100, &rig, arena);
}

int morb_ba_problem_create_fisheye(morb_optimizer* o, morb_ba_problem** out, int nKF, const float* kfPose, const uint8_t* kfFixed,
                                   int nMP, const float* mpPos, int nE, const int* eKF, const int* eMP, const float* eObs2,
                                   const uint8_t* eRight, const float* eInvSigma2, const float* camL8, const float* camR8,
                                   const float* Trl7, int lambdaInit100) {
  return ba_problem_create_fisheye(o, out, nKF, kfPose, kfFixed, nMP, mpPos, nE, eKF, eMP, eObs2, eRight, eInvSigma2, camL8, camR8, Trl7,
                                   lambdaInit100, false);
}

int morb_ba_set_mode(morb_ba_problem* p, int mode) {
  MORB_REQUIRE(p && (mode == 0 || mode == 1), MORB_ERR_INVALID, "mode must be 0 (grid) or 1 (persistent workgroup)");
  p->mode = mode;
  return MORB_OK;
}

int morb_ba_set_stop(morb_ba_problem* p, int stop) {
  MORB_REQUIRE(p, MORB_ERR_INVALID, "NULL problem");
  // No HIP call: the flag lives in pinned host memory that the device maps, so it lands while a solve is running on any
  // stream (a copy on the null stream would wait for the very kernels it is meant to stop) and from any thread.
  __atomic_store_n(p->h_stop, stop ? 1 : 0, __ATOMIC_RELEASE);
  return MORB_OK;
}

int morb_ba_solve(morb_ba_problem* p, void* stream) {
  MORB_REQUIRE(p, MORB_ERR_INVALID, "NULL problem");
  MORB_ENTER(st, p->opt, stream);
  MORB_HIP_CHECK(p->solved.create(hipEventDisableTiming));
  struct RecordOnExit { hipEvent_t ev; hipStream_t st; ~RecordOnExit() { (void)hipEventRecord(ev, st); } } recordOnExit{p->solved, st};
  const int n = std::max(p->h.nKF, p->h.nMP * 3);
  hipLaunchKernelGGL(k_ba_reset, dim3(div_up(n, 256)), dim3(256), 0, st, p->h, p->d_pose0, p->d_pt0);
  if (p->mode == 1) {
    hipLaunchKernelGGL(k_local_ba, dim3(1), dim3(BA_T), p->ldsBytes, st, p->d_desc, p->useLds);
    MORB_HIP_CHECK(hipGetLastError());
    return MORB_OK;
  }
  // ---- grid mode, LM control flow on the device: a slot is one trial (its seven launches as one hipGraph: 0.89 -> 0.95 ms per solve, profiles/r04/README.md) ----
  const BaDev& h = p->h;
  const BaDev* d = p->d_desc;
  const int rb = p->redBlocks, kfBlocks = div_up(std::max(h.nChunks, 1), 4);
  return ba_queue_solve(p, st, 100, "LocalBundleAdjustment", [&](int slot) {
    if (!slot) hipLaunchKernelGGL(k_g_chi2, dim3(rb), dim3(GB), 0, st, d, h.redPart, (const double*)(h.redPart + rb), 2);   // the first chi2 and lambda
    // buildSystem (runs only when the previous trial was accepted): keyframe chunks and map points in one launch
    if (h.rig) hipLaunchKernelGGL(k_g_build<true>, dim3(kfBlocks + div_up(h.nMP, GB / MP_LANES)), dim3(GB), 0, st, d, kfBlocks);
    else hipLaunchKernelGGL(k_g_build<false>, dim3(kfBlocks + div_up(h.nMP, GB / MP_LANES)), dim3(GB), 0, st, d, kfBlocks);
    ba_launch_solve_phases(p, st);
    hipLaunchKernelGGL(k_g_chi2, dim3(rb), dim3(GB), 0, st, d, h.redPart, (const double*)(h.redPart + rb), 1);
  }, [&]() { hipLaunchKernelGGL(k_g_finish, dim3(rb), dim3(GB), 0, st, d, -1, -1); });
}

int morb_ba_schur_profile(morb_ba_problem* p, int iters, float* msPerLaunch, double* flops, double* usefulFlops) {
  MORB_REQUIRE(p && iters > 0 && msPerLaunch && flops && usefulFlops, MORB_ERR_INVALID, "bad argument");
  MORB_HIP_CHECK(hipSetDevice(p->opt->device));
  hipStream_t st = p->opt->stream;
  morb::Event e0, e1;
  MORB_HIP_CHECK(e0.create(hipEventDefault)); MORB_HIP_CHECK(e1.create(hipEventDefault));
  const morbschur::Plan& sp = p->schur;
  auto launch = [&]() { hipLaunchKernelGGL(morbschur::k_schur_mfma, dim3(sp.nblk, sp.nsplit), dim3(64), 0, st, (const double*)p->h.sWD, (const double*)p->h.sW, sp.Mp, sp.ksteps, sp.stepsPerSplit, p->h.sBlocks, p->h.sPart, (const int*)nullptr); };
  launch();
  MORB_HIP_CHECK(hipEventRecord(e0, st));
  for (int i = 0; i < iters; ++i) launch();
  MORB_HIP_CHECK(hipEventRecord(e1, st));
  MORB_HIP_CHECK(hipEventSynchronize(e1));
  float ms = 0;
  MORB_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  *msPerLaunch = ms / iters;
  *flops = 2.0 * sp.nblk * morbschur::SB * morbschur::SB * (double)sp.nsplit * sp.stepsPerSplit * 4;
  *usefulFlops = 2.0 * 6 * 3 * (3 + 6) * (double)p->nPairEntries;   // per (e1, e2) entry: B1 D^-1 (6x3x3) and (B1 D^-1) B2^T (6x3x6)
  return MORB_OK;
}

int morb_ba_results(morb_ba_problem* p, float* kfPose, float* mpPos, uint8_t* eraseFlag, int* stats2) {
  MORB_REQUIRE(p, MORB_ERR_INVALID, "NULL problem");
  MORB_HIP_CHECK(hipSetDevice(p->opt->device));
  // the solve may have run on a caller's stream: wait for THAT stream (not for the device: with the reference's threading a tracked
  // frame's optimisation on another handle must not wait for this solve, nor this copy for it), then copy on the handle's own stream
  // (a copy on the null stream would also wait for, and hold up, every other handle's blocking stream)
  if (p->solved) MORB_HIP_CHECK(hipEventSynchronize(p->solved));
  hipStream_t st = p->opt->stream;
  MORB_HIP_CHECK(ba_queue_results(p, st, kfPose, mpPos, eraseFlag));
  if (stats2) MORB_HIP_CHECK(hipMemcpyAsync(stats2, p->h.stats, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipStreamSynchronize(st));
  return MORB_OK;
}

// the one-shot LocalBundleAdjustment behind its create call (p lives in the handle's workspace for the duration of the call)
static int local_ba_solve_once(morb_ba_problem* p, const unsigned char* stopFlag, float* kfPose, float* mpPos, uint8_t* eraseFlag, int* stats2) {
  p->userStop = stopFlag;   // optimizer.setForceStopFlag(pbStopFlag) (:1142): the LM loop polls the caller's flag at every iteration and trial
  int rc = morb_ba_solve(p, nullptr);
  if (rc == MORB_OK) rc = morb_ba_results(p, kfPose, mpPos, eraseFlag, stats2);
  morb_ba_problem_destroy(p);
  return rc;
}

int morb_local_bundle_adjustment(morb_optimizer* o, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos,
                                 int nE, const int* eKF, const int* eMP, const float* eObs, const float* eInvSigma2,
                                 float fx, float fy, float cx, float cy, float bf, int lambdaInit100,
                                 const unsigned char* stopFlag, uint8_t* eraseFlag, int* stats2) {
  if (stopFlag && *(const volatile unsigned char*)stopFlag) { if (stats2) stats2[0] = stats2[1] = 0; return MORB_OK; }  // :1355-1356
  morb_ba_problem* p = nullptr;
  const int rc = ba_problem_create(o, &p, nKF, kfPose, kfFixed, nMP, mpPos, nE, eKF, eMP, eObs, eInvSigma2, fx, fy, cx, cy, bf, lambdaInit100,
                                   nullptr, true);
  return rc != MORB_OK ? rc : local_ba_solve_once(p, stopFlag, kfPose, mpPos, eraseFlag, stats2);
}

int morb_local_bundle_adjustment_fisheye(morb_optimizer* o, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos,
                                         int nE, const int* eKF, const int* eMP, const float* eObs2, const uint8_t* eRight,
                                         const float* eInvSigma2, const float* camL8, const float* camR8, const float* Trl7,
                                         int lambdaInit100, const unsigned char* stopFlag, uint8_t* eraseFlag, int* stats2) {
  if (stopFlag && *(const volatile unsigned char*)stopFlag) { if (stats2) stats2[0] = stats2[1] = 0; return MORB_OK; }  // :1355-1356
  morb_ba_problem* p = nullptr;
  const int rc = ba_problem_create_fisheye(o, &p, nKF, kfPose, kfFixed, nMP, mpPos, nE, eKF, eMP, eObs2, eRight, eInvSigma2, camL8, camR8, Trl7,
                                           lambdaInit100, true);
  return rc != MORB_OK ? rc : local_ba_solve_once(p, stopFlag, kfPose, mpPos, eraseFlag, stats2);
}

// ---- the welding BA of map merging (k_mg_*): both rounds, the classification between them and the flags as one queue of launches ----
static int merge_ba_solve(morb_ba_problem* p, const MergeDev& mh) {
  MORB_ENTER(st, p->opt, nullptr);
  const BaDev& h = p->h;
  const MergeDev* dm = reinterpret_cast<const MergeDev*>(p->d_desc);   // (its first member is the BaDev the shared phase kernels read)
  const int rb = p->redBlocks;
  const int n = std::max(h.nKF, h.nMP * 3);
  hipLaunchKernelGGL(k_ba_reset, dim3(div_up(n, 256)), dim3(256), 0, st, p->h, p->d_pose0, p->d_pt0);
  hipLaunchKernelGGL(k_mg_reset, dim3(1), dim3(64), 0, st, mh);
  const int kfBlocks = div_up(std::max(h.nChunks, 1), 4);
  // a slot is one trial, or the hand-over between the rounds: at most 5 x 10 trials, the hand-over, 10 x 10 trials
  return ba_queue_solve(p, st, 160, "merge LocalBundleAdjustment", [&](int slot) {
    if (!slot) hipLaunchKernelGGL(k_mg_chi2, dim3(rb), dim3(GB), 0, st, dm, h.redPart, (const double*)(h.redPart + rb), 2);
    if (h.rig) hipLaunchKernelGGL(k_mg_build<true>, dim3(kfBlocks + div_up(h.nMP, GB / MP_LANES)), dim3(GB), 0, st, dm, kfBlocks);
    else hipLaunchKernelGGL(k_mg_build<false>, dim3(kfBlocks + div_up(h.nMP, GB / MP_LANES)), dim3(GB), 0, st, dm, kfBlocks);
    ba_launch_solve_phases(p, st);
    hipLaunchKernelGGL(k_mg_chi2, dim3(rb), dim3(GB), 0, st, dm, h.redPart, (const double*)(h.redPart + rb), 1);
  }, [&]() { hipLaunchKernelGGL(k_mg_finish, dim3(rb), dim3(GB), 0, st, dm); });
}

static int merge_ba_once(morb_optimizer* o, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos, int nE, const int* eKF,
                         const int* eMP, const float* eObs3, const float* eInvSigma2, const Cam& cam, const Rig* rig, const uint8_t* stopFlag,
                         uint8_t* eraseFlag, uint8_t* levelFlag, int* stats6) {
  // (ahead of the stop flag: a refused call is refused whatever the flag says, and before any upload or launch)
  MORB_REQUIRE(eraseFlag && stats6, MORB_ERR_INVALID, "NULL argument");
  if (const int rc = ba_check_graph(o, nKF, kfPose, kfFixed, nMP, mpPos, nE, eKF, eMP, eObs3, eInvSigma2)) return rc;
  if (stopFlag && *(const volatile uint8_t*)stopFlag) {   // :3650-3651: nothing is optimised, nothing written
    for (int k = 0; k < 6; ++k) stats6[k] = 0;
    return MORB_OK;
  }
  MergeDev mh;
  memset(&mh, 0, sizeof mh);
  mh.deltaMono = (double)(float)sqrt(5.99); mh.deltaStereo = (double)(float)sqrt(7.815);   // thHuber2D / thHuber3D (:3547-3548)
  morb_ba_problem* p = nullptr;
  int rc = ba_problem_create(o, &p, nKF, kfPose, kfFixed, nMP, mpPos, nE, eKF, eMP, eObs3, eInvSigma2, cam.fx, cam.fy, cam.cx, cam.cy, cam.bf, 0,
                             rig, true, &mh);
  if (rc != MORB_OK) return rc;
  p->userStop = stopFlag;   // optimizer.setForceStopFlag(pbStopFlag) (:3452)
  rc = merge_ba_solve(p, mh);
  hipStream_t st = o->stream;
  if (rc == MORB_OK) {
    hipError_t e = ba_queue_results(p, st, kfPose, mpPos, eraseFlag);
    if (e == hipSuccess && levelFlag) e = hipMemcpyAsync(levelFlag, mh.level, nE, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(stats6, mh.stats6, sizeof(int) * 6, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { set_error("merge LocalBundleAdjustment: %s", hipGetErrorString(e)); rc = MORB_ERR_HIP; }
  }
  morb_ba_problem_destroy(p);   // (waits for the handle's stream: the workspace is free for the next call)
  return rc;
}

int morb_merge_bundle_adjustment(morb_optimizer* o, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos, int nE,
                                 const int* eKF, const int* eMP, const float* eObs, const float* eInvSigma2, float fx, float fy, float cx,
                                 float cy, float bf, const uint8_t* stopFlag, uint8_t* eraseFlag, uint8_t* levelFlag, int* stats6) {
  return merge_ba_once(o, nKF, kfPose, kfFixed, nMP, mpPos, nE, eKF, eMP, eObs, eInvSigma2, Cam{fx, fy, cx, cy, bf}, nullptr, stopFlag,
                       eraseFlag, levelFlag, stats6);
}

int morb_merge_bundle_adjustment_fisheye(morb_optimizer* o, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos, int nE,
                                         const int* eKF, const int* eMP, const float* eObs2, const float* eInvSigma2, const float* camL8,
                                         const uint8_t* stopFlag, uint8_t* eraseFlag, uint8_t* levelFlag, int* stats6) {
  MORB_REQUIRE(eObs2 && camL8, MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nE > 0, MORB_ERR_INVALID, "empty problem");
  // every edge is an EdgeSE3ProjectXYZ with pKF->mpCamera, the left KB8 camera (:3582-3602)
  const std::vector<float> obs3 = fisheye_obs3(nE, eObs2, nullptr);
  const float Trl7[7] = {0, 0, 0, 1, 0, 0, 0};   // (no right-camera edge reads the second camera or mTrl)
  const Rig rig = make_rig(camL8, camL8, Trl7);
  return merge_ba_once(o, nKF, kfPose, kfFixed, nMP, mpPos, nE, eKF, eMP, obs3.data(), eInvSigma2, Cam{0.f, 0.f, 0.f, 0.f, 0.f}, &rig, stopFlag,
                       eraseFlag, levelFlag, stats6);
}

}  // extern "C"
