// Optimizer::BundleAdjustment (reference src/Optimizer.cc:56-362) for MI355X (gfx950): the whole-map bundle adjustment LoopClosing runs behind
// a loop closure (GlobalBundleAdjustemnt, LoopClosing.cc:2302) — every keyframe and every point of the map, g2o's Levenberg-Marquardt over
// BlockSolver_6_3 with the edges of optimizer_device.h.  What sets it apart from LocalBundleAdjustment (local_ba.hip) is its size: the reduced
// camera system has a 6 x 6 block row per keyframe of the map, so neither a dense [3 nMP][6 nKF] Schur operand nor a dense LDL^T fits.
//   * k_gba_linearize: error, Huber weight and both Jacobians of every edge, a lane per edge (EdgeSE3ProjectXYZ, EdgeStereoSE3ProjectXYZ,
//     EdgeSE3ProjectXYZToBody; the kernels as :171-175, :204-208, :244-246 set them).
//   * k_gba_assemble: Hpp and bp per keyframe, Hll and bl per point, Hpl per distinct (point, free keyframe) pair, every entry summed over
//     its edges in edge order: no floating-point atomics.
//   * k_gba_maxdiag: computeLambdaInit — 1e-5 * max |H_jj| over the pose and the point diagonals of the first system; no user lambda.
//   * k_gba_dinv: Dinv = (Hll + lambda I)^-1 per point, Hpl Dinv and Hpl Dinv bl per pair.
//   * k_gba_schur / k_gba_schur_finish: the sparse Schur complement.  An envelope block (i1, i2) is Hpp (on the diagonal) minus the sum over
//     the points both keyframes see of (Hpl_i1 Dinv) Hpl_i2^T, in point order (block_solver.hpp:354-480); its contribution list is cut into
//     chunks of GBA_CHUNK, a lane per (chunk, entry) over the whole grid, and the chunks' sums are added in order.  Nothing dense in
//     nMP x nKF exists.
//   * k_gba_factor: H + lambda I = L D L^T over the envelope of the 6 x 6 block rows (envelope_plan.h) by envelope_ldlt.h, which describes
//     the schedule: GBA_ROWS covering rows take one pass, GBA_STAGE blocks are staged at a time.  A zero or NaN pivot is a failed
//     factorisation: a rejected trial.
//   * k_gba_backsub / k_gba_points: the backward substitution (envelope_ldlt.h) and SE3Quat::exp(dx) * T; xl = Dinv (bl - Hpl^T xp) and +=
//     per point.
//   * k_gba_errors / k_gba_decide: robust chi2 per edge, summed by lane slices; g2o's Levenberg-Marquardt decisions (lm_control.h:
//     lm_decide_trial), optimize(nIterations), the stop flag polled at every decision, the host queueing trials through ba_host.h's
//     lm_slot_queue.
// A keyframe without an edge, a fixed keyframe and a point without an edge are not in the system and keep their bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
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
#include "optimizer_device.h"

namespace {

using namespace morb;

constexpr int GBA_NT = 256;                 // lanes of a workgroup
constexpr int GBA_ROWS = GBA_NT / 6;        // covering rows of 6 lines one pass of envelope_factor takes (the diagonal block's among them): 42
constexpr int GBA_STAGE = 64;               // blocks of the column's own row envelope_factor stages in LDS at a time (18 KiB)
constexpr int GBA_CHUNK = 64;               // Schur contributions one lane adds before the chunks are added
// envelope blocks a handle may grow to: the bytes the Sim3 pose graph allows its 7 x 7 envelope (2^22 blocks of H and of L), in 6 x 6 blocks
constexpr size_t GBA_MAX_BLOCKS = ((size_t)1 << 22) * 49 / 36;
constexpr int GBA_EDGE = 31;                // doubles of an edge's record: Jp 3 x 6, Jl 3 x 3, -(w info) e, w info
enum { GE_JP = 0, GE_JL = 18, GE_RW = 27, GE_WO = 30 };

struct GbaDev {
  int nKF, nMP, nE, n, nBlocks, nPairs, nChunks, maxIts, robust;
  const int *eKF, *eMP;                 // [nE]
  const float *eObs, *eInfo;            // [nE][3] (x, y, uRight; on the rig -2 = left camera, -3 = ToBody), [nE]
  const int* col;                       // [nKF] block row of the system, -1: fixed or without an edge
  const int* rowKF;                     // [n] its keyframe
  const int *kfStart, *kfEdges;         // edges by keyframe index, in edge order (free keyframes only)
  const int *mpStart, *mpEdges;         // edges by point, in edge order
  const int *pairStart, *pairEdges;     // [nPairs + 1] edges of a (point, free keyframe) pair, in edge order
  const int *pairCol, *pairMp;          // [nPairs]
  const int* mpPairStart;               // [nMP + 1] pairs are numbered by point, then by block row
  const int *kfPairStart, *kfPairs;     // [n + 1] pairs of a block row, in point order
  const int *rowFirst, *rowOff, *colStart, *colRows;   // envelope_plan.h
  const int* blkDiag;                   // [nBlocks] the block row of a diagonal block, else -1
  const int *chunkStart, *chunkEnd;     // [nChunks] positions in ct
  const int* blkChunkStart;             // [nBlocks + 1]
  const int2* ct;                       // Schur contributions (pair of the block's row, pair of its column), by envelope block, in point order
  double *pose, *poseT;                 // [nKF][7] current and trial
  double *pt, *ptT;                     // [nMP][3]
  double* E;                            // [nE][GBA_EDGE]
  double *Hpp, *bp;                     // [n][36], [6 n]
  double *Hll, *bl, *Dinv, *xl;         // [nMP][9], [nMP][3], [nMP][9], [nMP][3]
  double *Hpl, *HplD, *g;               // [nPairs][18] row-major 6 x 3; Hpl Dinv; [nPairs][6] Hpl Dinv bl
  double* part;                         // [nChunks][36]
  double *H, *L;                        // [nBlocks][36] the reduced system in the envelope; its factor
  double *b, *y, *x, *d;                // [6 n]
  double* chiE;                         // [nE]
  LmControl* lm;
  double* chi2;                         // [2]
  int* lmi;                             // [8] LMW_* (lm_control.h)
  int* lmHost;                          // mapped host words: [0] decided trials, [1] done, [2] the caller's stop flag as the host forwards it
  Cam cam;
  const Rig* rig;
  double deltaMono, deltaStereo;
};

__device__ __forceinline__ SE3 gba_load(const double* p) {
  SE3 s;
#pragma unroll
  for (int i = 0; i < 4; ++i) s.q[i] = p[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) s.t[i] = p[4 + i];
  return s;
}
__device__ __forceinline__ void gba_inv3(const double* m, double* o) {
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double id = 1.0 / (m[0] * c00 + m[1] * c01 + m[2] * c02);
  o[0] = c00 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  o[3] = c01 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  o[6] = c02 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}
// the Huber delta of an edge, 0: no kernel.  A ToBody edge carries one whatever bRobust says (:244-246)
__device__ __forceinline__ double gba_delta(const GbaDev& D, const float* o) {
  if (D.rig && o[2] < -2.5f) return D.deltaMono;
  if (!D.robust) return 0.0;
  return o[2] < 0 ? D.deltaMono : D.deltaStereo;
}
__device__ __forceinline__ bool gba_stop(const GbaDev& D) { return __hip_atomic_load(D.lmHost + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0; }

// linearizeOplus and the robust weight of every edge at the current estimate
template <bool RIG>
__global__ __launch_bounds__(GBA_NT) void k_gba_linearize(GbaDev D) {
  if (D.lmi[LMW_DONE] || !D.lmi[LMW_REBUILD]) return;
  const int e = blockIdx.x * GBA_NT + threadIdx.x;
  if (e >= D.nE) return;
  const SE3 T = gba_load(D.pose + 7 * (size_t)D.eKF[e]);
  const float* o = D.eObs + 3 * (size_t)e;
  const bool st = !(o[2] < 0);
  const double info = (double)D.eInfo[e];
  double xc[3], err[3], w = 1.0, R[9], Jp[18], Jl[9];
  se3_map(T, D.pt + 3 * (size_t)D.eMP[e], xc);
  const double c = ba_edge_error(D.cam, D.rig, st, xc, o, info, err);
  const double delta = gba_delta(D, o);
  if (delta > 0) huber(delta, c, &w);
  q_to_R(T.q, R);
  ba_edge_jac<RIG>(D.cam, D.rig, st, xc, o, R, Jp, Jl);
  double* out = D.E + (size_t)e * GBA_EDGE;
#pragma unroll
  for (int k = 0; k < 18; ++k) out[GE_JP + k] = Jp[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) out[GE_JL + k] = Jl[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) out[GE_RW + k] = -info * err[k] * w;
  out[GE_WO] = w * info;
}

// sum over the edges list[k0 .. k1) of (A^T wo B)(r, c), A = the record's Jacobian at offset oa with sa columns, B likewise; in edge order
__device__ __forceinline__ double gba_sum_jtj(const double* E, const int* list, int k0, int k1, int oa, int sa, int r, int ob, int sb, int c) {
  double acc = 0;
  for (int k = k0; k < k1; ++k) {
    const double* rec = E + (size_t)list[k] * GBA_EDGE;
    const double wo = rec[GE_WO];
    double h = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) h += rec[oa + i * sa + r] * wo * rec[ob + i * sb + c];
    acc += h;
  }
  return acc;
}
__device__ __forceinline__ double gba_sum_jtr(const double* E, const int* list, int k0, int k1, int oa, int sa, int r) {
  double acc = 0;
  for (int k = k0; k < k1; ++k) {
    const double* rec = E + (size_t)list[k] * GBA_EDGE;
    double s = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) s += rec[oa + i * sa + r] * rec[GE_RW + i];
    acc += s;
  }
  return acc;
}

// Hpp, bp (42 lanes per block row), Hll, bl (12 per point), Hpl (18 per pair)
__global__ __launch_bounds__(GBA_NT) void k_gba_assemble(GbaDev D) {
  if (D.lmi[LMW_DONE] || !D.lmi[LMW_REBUILD]) return;
  size_t gid = (size_t)blockIdx.x * GBA_NT + threadIdx.x;
  if (gid < (size_t)D.n * 42) {
    const int a = (int)(gid / 42), k = (int)(gid % 42), kf = D.rowKF[a];
    const int k0 = D.kfStart[kf], k1 = D.kfStart[kf + 1];
    if (k < 36) D.Hpp[(size_t)a * 36 + k] = gba_sum_jtj(D.E, D.kfEdges, k0, k1, GE_JP, 6, k / 6, GE_JP, 6, k % 6);
    else D.bp[(size_t)a * 6 + k - 36] = gba_sum_jtr(D.E, D.kfEdges, k0, k1, GE_JP, 6, k - 36);
    return;
  }
  gid -= (size_t)D.n * 42;
  if (gid < (size_t)D.nMP * 12) {
    const int m = (int)(gid / 12), k = (int)(gid % 12);
    const int k0 = D.mpStart[m], k1 = D.mpStart[m + 1];
    if (k < 9) D.Hll[(size_t)m * 9 + k] = gba_sum_jtj(D.E, D.mpEdges, k0, k1, GE_JL, 3, k / 3, GE_JL, 3, k % 3);
    else D.bl[(size_t)m * 3 + k - 9] = gba_sum_jtr(D.E, D.mpEdges, k0, k1, GE_JL, 3, k - 9);
    return;
  }
  gid -= (size_t)D.nMP * 12;
  if (gid < (size_t)D.nPairs * 18) {
    const int p = (int)(gid / 18), k = (int)(gid % 18);
    D.Hpl[gid] = gba_sum_jtj(D.E, D.pairEdges, D.pairStart[p], D.pairStart[p + 1], GE_JP, 6, k / 3, GE_JL, 3, k % 3);
  }
}

// computeLambdaInit behind the first assembly.  One workgroup; a maximum has no order.
__global__ __launch_bounds__(GBA_NT) void k_gba_maxdiag(GbaDev D) {
  __shared__ double sMax[GBA_NT];
  if (D.lmi[LMW_DONE] || !D.lmi[LMW_LAMBDA0]) return;
  const int t = threadIdx.x;
  double m = 0;
  for (int i = t; i < 6 * D.n; i += GBA_NT) m = fmax(m, fabs(D.Hpp[(size_t)(i / 6) * 36 + (i % 6) * 7]));
  for (int i = t; i < 3 * D.nMP; i += GBA_NT) m = fmax(m, fabs(D.Hll[(size_t)(i / 3) * 9 + (i % 3) * 4]));
  sMax[t] = m;
  __syncthreads();
  for (int w = GBA_NT / 2; w > 0; w >>= 1) {
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

// Dinv per point; Hpl Dinv and Hpl Dinv bl per pair (a pair's lane inverts its point's block itself)
__global__ __launch_bounds__(GBA_NT) void k_gba_dinv(GbaDev D) {
  if (D.lmi[LMW_DONE]) return;
  const int gid = blockIdx.x * GBA_NT + threadIdx.x;
  if (gid >= D.nMP + D.nPairs) return;
  const double lambda = D.lm->lambda;
  const int p = gid - D.nMP, m = gid < D.nMP ? gid : D.pairMp[p];
  double Hl[9], Di[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Hl[k] = D.Hll[(size_t)m * 9 + k];
  Hl[0] += lambda; Hl[4] += lambda; Hl[8] += lambda;
  gba_inv3(Hl, Di);
  if (gid < D.nMP) {
    const bool has = D.mpStart[m + 1] > D.mpStart[m];
#pragma unroll
    for (int k = 0; k < 9; ++k) D.Dinv[(size_t)m * 9 + k] = has ? Di[k] : 0.0;
    return;
  }
  const double* W = D.Hpl + (size_t)p * 18;
  const double* bl = D.bl + (size_t)m * 3;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double wd[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) wd[j] = W[i * 3] * Di[j] + W[i * 3 + 1] * Di[3 + j] + W[i * 3 + 2] * Di[6 + j];
#pragma unroll
    for (int j = 0; j < 3; ++j) D.HplD[(size_t)p * 18 + i * 3 + j] = wd[j];
    D.g[(size_t)p * 6 + i] = wd[0] * bl[0] + wd[1] * bl[1] + wd[2] * bl[2];
  }
}

// a chunk of an envelope block's contributions: sum of (Hpl_i1 Dinv) Hpl_i2^T, a lane per (chunk, entry), in point order
__global__ __launch_bounds__(GBA_NT) void k_gba_schur(GbaDev D) {
  if (D.lmi[LMW_DONE]) return;
  const size_t gid = (size_t)blockIdx.x * GBA_NT + threadIdx.x;
  if (gid >= (size_t)D.nChunks * 36) return;
  const int c = (int)(gid / 36), ent = (int)(gid % 36), r = ent / 6, cc = ent % 6;
  double acc = 0;
  for (int q = D.chunkStart[c]; q < D.chunkEnd[c]; ++q) {
    const int2 pr = D.ct[q];
    const double* A = D.HplD + (size_t)pr.x * 18 + r * 3;
    const double* B = D.Hpl + (size_t)pr.y * 18 + cc * 3;
    acc += A[0] * B[0] + A[1] * B[1] + A[2] * B[2];
  }
  D.part[gid] = acc;
}

// the reduced system: H = Hpp - the chunks' sums in order, b = bp - sum Hpl Dinv bl over the block row's pairs in point order
__global__ __launch_bounds__(GBA_NT) void k_gba_schur_finish(GbaDev D) {
  if (D.lmi[LMW_DONE]) return;
  const size_t gid = (size_t)blockIdx.x * GBA_NT + threadIdx.x;
  const size_t nH = (size_t)D.nBlocks * 36;
  if (gid < nH) {
    const int blk = (int)(gid / 36), ent = (int)(gid % 36);
    double acc = 0;
    for (int c = D.blkChunkStart[blk]; c < D.blkChunkStart[blk + 1]; ++c) acc += D.part[(size_t)c * 36 + ent];
    const int a = D.blkDiag[blk];
    D.H[gid] = (a >= 0 ? D.Hpp[(size_t)a * 36 + ent] : 0.0) - acc;
    return;
  }
  const size_t k = gid - nH;
  if (k >= (size_t)D.n * 6) return;
  const int a = (int)(k / 6), r = (int)(k % 6);
  double acc = 0;
  for (int q = D.kfPairStart[a]; q < D.kfPairStart[a + 1]; ++q) acc += D.g[(size_t)D.kfPairs[q] * 6 + r];
  D.b[k] = D.bp[k] - acc;
}

// H + lambda I = L D L^T over the envelope, and y = L^-1 b on the way (envelope_ldlt.h).  One workgroup.  A zero or NaN pivot fails.
__global__ __launch_bounds__(GBA_NT) void k_gba_factor(GbaDev D) {
  if (D.lmi[LMW_DONE]) return;
  const bool ok = envelope_factor<6, GBA_NT, GBA_STAGE, 1, false>(envelope_sys(D), D.lm->lambda);
  if (threadIdx.x == 0) D.lmi[LMW_OK2] = ok ? 1 : 0;
}

// x = L^-T D^-1 y (envelope_ldlt.h), then the trial poses SE3Quat::exp(x_v) * T_v.  One workgroup.  A failed factorisation leaves the
// step zero.
__global__ __launch_bounds__(GBA_NT) void k_gba_backsub(GbaDev D) {
  if (D.lmi[LMW_DONE]) return;
  const int t = threadIdx.x, n = D.n;
  if (D.lmi[LMW_OK2]) {
    envelope_backsub<6, GBA_NT>(envelope_sys(D));
  } else {
    for (int i = t; i < 6 * n; i += GBA_NT) D.x[i] = 0.0;
    __threadfence_block();
    __syncthreads();
  }
  for (int v = t; v < D.nKF; v += GBA_NT) {
    const int a = D.col[v];
    SE3 T = gba_load(D.pose + 7 * (size_t)v);
    if (a >= 0) {
      double u[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) u[k] = D.x[(size_t)a * 6 + k];
      T = se3_mul(se3_exp(u), T);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) D.poseT[7 * (size_t)v + k] = T.q[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) D.poseT[7 * (size_t)v + 4 + k] = T.t[k];
  }
}

// xl = Dinv (bl - Hpl^T xp) over the point's pairs in order, and the trial points
__global__ __launch_bounds__(GBA_NT) void k_gba_points(GbaDev D) {
  if (D.lmi[LMW_DONE]) return;
  const int m = blockIdx.x * GBA_NT + threadIdx.x;
  if (m >= D.nMP) return;
  double xl[3] = {0, 0, 0};
  if (D.lmi[LMW_OK2] && D.mpStart[m + 1] > D.mpStart[m]) {
    double cl[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) cl[j] = D.bl[(size_t)m * 3 + j];
    for (int p = D.mpPairStart[m]; p < D.mpPairStart[m + 1]; ++p) {
      const double* W = D.Hpl + (size_t)p * 18;
      const double* xp = D.x + (size_t)D.pairCol[p] * 6;
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 6; ++i) cl[j] -= W[i * 3 + j] * xp[i];
    }
    const double* Di = D.Dinv + (size_t)m * 9;
#pragma unroll
    for (int j = 0; j < 3; ++j) xl[j] = Di[j * 3] * cl[0] + Di[j * 3 + 1] * cl[1] + Di[j * 3 + 2] * cl[2];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) { D.xl[(size_t)m * 3 + j] = xl[j]; D.ptT[(size_t)m * 3 + j] = D.pt[(size_t)m * 3 + j] + xl[j]; }
}

// computeError and the robust chi2 of every edge at the trial estimate (trial != 0) or at the current one
__global__ __launch_bounds__(GBA_NT) void k_gba_errors(GbaDev D, int trial) {
  if (D.lmi[LMW_DONE]) return;
  const int e = blockIdx.x * GBA_NT + threadIdx.x;
  if (e >= D.nE) return;
  const double *pose = trial ? D.poseT : D.pose, *pt = trial ? D.ptT : D.pt;
  const float* o = D.eObs + 3 * (size_t)e;
  double xc[3], err[3], w;
  se3_map(gba_load(pose + 7 * (size_t)D.eKF[e]), pt + 3 * (size_t)D.eMP[e], xc);
  const double c = ba_edge_error(D.cam, D.rig, !(o[2] < 0), xc, o, (double)D.eInfo[e], err);
  const double delta = gba_delta(D, o);
  D.chiE[e] = delta > 0 ? huber(delta, c, &w) : c;
}

// init != 0: behind the first computeActiveErrors; else g2o's decision after a trial (lm_control.h).  One workgroup.
__global__ __launch_bounds__(GBA_NT) void k_gba_decide(GbaDev D, int init) {
  __shared__ double buf[GBA_NT];
  __shared__ int sKeep;
  if (D.lmi[LMW_DONE]) return;
  const int t = threadIdx.x;
  const double chi = lm_sum_of_lane_slices<GBA_NT>(buf, D.nE, [&](int e) { return D.chiE[e]; });
  LmControl c = *D.lm;
  if (init) {
    if (t == 0) {
      const int stop = gba_stop(D) ? 1 : 0;   // (raised between the entry and the first iteration: optimize() ends before it)
      lm_iteration(c, chi);   // (lambda comes behind the first assembly: k_gba_maxdiag)
      *D.lm = c;
      D.chi2[0] = chi; D.chi2[1] = chi;
      D.lmi[LMW_REBUILD] = 1; D.lmi[LMW_ITS] = 0; D.lmi[LMW_TRIALS] = 0; D.lmi[LMW_OK2] = 1; D.lmi[LMW_LAMBDA0] = 1; D.lmi[LMW_DONE] = stop;
      if (stop) __hip_atomic_store(D.lmHost + 1, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return;
  }
  const double lambda = c.lambda;
  const double gainP = lm_sum_of_lane_slices<GBA_NT>(buf, 6 * D.n, [&](int i) { return D.x[i] * (lambda * D.x[i] + D.bp[i]); });   // computeScale()
  const double gainL = lm_sum_of_lane_slices<GBA_NT>(buf, 3 * D.nMP, [&](int i) { return D.xl[i] * (lambda * D.xl[i] + D.bl[i]); });
  if (t == 0) sKeep = lm_decide_trial(c, chi, D.lmi[LMW_OK2] != 0, gainP + gainL, gba_stop(D), D.maxIts, D.lm, D.chi2, D.lmi, D.lmHost) ? 1 : 0;
  __syncthreads();
  if (sKeep) {
    for (int i = t; i < 7 * D.nKF; i += GBA_NT) D.pose[i] = D.poseT[i];
    for (int i = t; i < 3 * D.nMP; i += GBA_NT) D.pt[i] = D.ptT[i];
  }
}

int gba_run(morb_optimizer* o, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos, int nE, const int* eKF, const int* eMP,
            const float* eObs3, const float* eInvSigma2, const Cam& cam, const Rig* rig, int nIterations, int bRobust, const uint8_t* stopFlag,
            int* stats4, double* chi2) {
  MORB_REQUIRE(o && kfPose && kfFixed && mpPos && eKF && eMP && eObs3 && eInvSigma2 && stats4 && chi2, MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nKF > 0 && nMP > 0 && nE > 0, MORB_ERR_INVALID, "empty problem");
  MORB_REQUIRE(nIterations >= 1 && nIterations <= 100, MORB_ERR_INVALID, "nIterations outside 1 .. 100");
  auto finite = [](const float* p, size_t n) {
    for (size_t k = 0; k < n; ++k) if (!std::isfinite(p[k])) return false;
    return true;
  };
  MORB_REQUIRE(finite(kfPose, (size_t)7 * nKF) && finite(mpPos, (size_t)3 * nMP), MORB_ERR_INVALID, "a non-finite pose or point");
  MORB_REQUIRE(finite(eObs3, (size_t)3 * nE) && finite(eInvSigma2, nE), MORB_ERR_INVALID, "a non-finite observation or information");
  for (int e = 0; e < nE; ++e) MORB_REQUIRE(eKF[e] >= 0 && eKF[e] < nKF && eMP[e] >= 0 && eMP[e] < nMP, MORB_ERR_INVALID, "edge index out of range");
  // ---- the symbolic pass: which keyframes are in the system, the (point, free keyframe) pairs, the envelope, the Schur contributions ----
  std::vector<uint8_t> fixed(nKF);
  for (int v = 0; v < nKF; ++v) fixed[v] = kfFixed[v] ? 1 : 0;
  std::vector<int> mpStart, mpEdges;
  csr_by_key(eMP, nE, nMP, mpStart, mpEdges);
  // per point, its free keyframes ascending and without repeats: (keyframe, edge) sorted by keyframe, then by edge
  std::vector<int> pairKF, pairMp, pairStart, pairEdges, mpPairStart(nMP + 1, 0);
  std::vector<int> envI, envJ;   // the covisible pairs that span the envelope: every free keyframe of a point with the point's lowest one
  {
    std::vector<std::pair<int, int>> ke;
    for (int m = 0; m < nMP; ++m) {
      ke.clear();
      for (int k = mpStart[m]; k < mpStart[m + 1]; ++k) if (!fixed[eKF[mpEdges[k]]]) ke.push_back({eKF[mpEdges[k]], mpEdges[k]});
      std::sort(ke.begin(), ke.end());
      for (size_t k = 0; k < ke.size(); ++k) {
        if (k == 0 || ke[k].first != ke[k - 1].first) {
          pairStart.push_back((int)pairEdges.size());
          pairKF.push_back(ke[k].first); pairMp.push_back(m);
          envI.push_back(ke[0].first); envJ.push_back(ke[k].first);
        }
        pairEdges.push_back(ke[k].second);
      }
      mpPairStart[m + 1] = (int)pairKF.size();
    }
    pairStart.push_back((int)pairEdges.size());
  }
  const int nPairs = (int)pairKF.size();
  auto nothing = [&]() {   // no free keyframe has an edge: nothing to optimise, nothing written
    for (int k = 0; k < 4; ++k) stats4[k] = 0;
    chi2[0] = chi2[1] = 0;
    return MORB_OK;
  };
  if (!nPairs) return nothing();
  EnvelopePlan P;
  const EnvelopeFit fit = plan_envelope(nKF, fixed.data(), nPairs, envI.data(), envJ.data(), GBA_MAX_BLOCKS, P);
  if (fit == EnvelopeFit::Empty) return nothing();
  MORB_REQUIRE(fit == EnvelopeFit::Ok, MORB_ERR_CAPACITY, "the envelope of the reduced camera system exceeds what the handle may grow to");
  const int n = P.n, nBlocks = P.nBlocks;
  size_t nCt = 0;
  for (int m = 0; m < nMP; ++m) { const size_t k = (size_t)(mpPairStart[m + 1] - mpPairStart[m]); nCt += k * (k + 1) / 2; }
  MORB_REQUIRE(nCt <= (size_t)INT_MAX, MORB_ERR_CAPACITY, "more Schur pair contributions than an int indexes");
  if (stopFlag && *(const volatile uint8_t*)stopFlag) {   // (behind the refusals: a refused call is refused whatever the flag says)
    for (int k = 0; k < 4; ++k) stats4[k] = 0;
    chi2[0] = chi2[1] = 0;
    return MORB_OK;
  }
  std::vector<int> pairCol(nPairs), rowKF(n), blkDiag(nBlocks, -1);
  for (int p = 0; p < nPairs; ++p) pairCol[p] = P.col[pairKF[p]];
  for (int v = 0; v < nKF; ++v) if (P.col[v] >= 0) rowKF[P.col[v]] = v;
  for (int a = 0; a < n; ++a) blkDiag[P.rowOff[a + 1] - 1] = a;
  std::vector<int> kfStart, kfEdges, kfPairStart, kfPairs;
  csr_by_key(eKF, nE, nKF, kfStart, kfEdges, P.col.data());
  csr_by_key(pairCol.data(), nPairs, n, kfPairStart, kfPairs);
  std::vector<int> ctStart, chunkKey, chunkStart, chunkEnd, blkChunkStart;
  std::vector<int2> ct(nCt);
  {
    std::vector<int> key(nCt), pos;
    std::vector<int2> item(nCt);
    size_t q = 0;
    for (int m = 0; m < nMP; ++m)
      for (int p1 = mpPairStart[m]; p1 < mpPairStart[m + 1]; ++p1)
        for (int p2 = mpPairStart[m]; p2 <= p1; ++p2) {   // (pairs ascend by block row within a point: p1's row >= p2's)
          const int a = pairCol[p1], b = pairCol[p2];
          key[q] = P.rowOff[a] + (b - P.rowFirst[a]);
          item[q].x = p1; item[q].y = p2;
          ++q;
        }
    csr_by_key(key.data(), (int)nCt, nBlocks, ctStart, pos);
    for (size_t k = 0; k < nCt; ++k) ct[k] = item[pos[k]];
    std::vector<int> all(nBlocks, 0);
    chunks_of(ctStart, all.data(), GBA_CHUNK, chunkKey, chunkStart, chunkEnd, &blkChunkStart);
  }
  const int nChunks = (int)chunkKey.size();
  std::vector<double> pose((size_t)7 * nKF), pt((size_t)3 * nMP);
  for (int v = 0; v < nKF; ++v) {   // g2o::SE3Quat(q.cast<double>(), t.cast<double>()) with its normalisation (:118-119)
    double q[4] = {kfPose[7 * v], kfPose[7 * v + 1], kfPose[7 * v + 2], kfPose[7 * v + 3]};
    if (q[3] < 0) for (double& c : q) c = -c;
    const double nn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    MORB_REQUIRE(nn > 0, MORB_ERR_INVALID, "a zero quaternion");
    for (int k = 0; k < 4; ++k) pose[(size_t)7 * v + k] = q[k] / nn;
    for (int k = 0; k < 3; ++k) pose[(size_t)7 * v + 4 + k] = kfPose[7 * v + 4 + k];
  }
  for (size_t k = 0; k < pt.size(); ++k) pt[k] = mpPos[k];

  MORB_ENTER(st, o, nullptr);
  GbaDev D;
  memset(&D, 0, sizeof D);
  D.nKF = nKF; D.nMP = nMP; D.nE = nE; D.n = n; D.nBlocks = nBlocks; D.nPairs = nPairs; D.nChunks = nChunks; D.maxIts = nIterations;
  D.robust = bRobust ? 1 : 0;
  D.cam = cam;
  D.deltaMono = (double)(float)sqrt(5.99); D.deltaStereo = (double)(float)sqrt(7.815);   // thHuber2D, thHuber3D (:126-127)
  ArenaCarver A;
  auto carve = [&]() {
    auto ints = [&](const std::vector<int>& v) { return (const int*)A.take(v.data(), sizeof(int) * v.size()); };
    D.eKF = (const int*)A.take(eKF, sizeof(int) * nE); D.eMP = (const int*)A.take(eMP, sizeof(int) * nE);
    D.eObs = (const float*)A.take(eObs3, sizeof(float) * 3 * nE); D.eInfo = (const float*)A.take(eInvSigma2, sizeof(float) * nE);
    D.col = ints(P.col); D.rowKF = ints(rowKF); D.kfStart = ints(kfStart); D.kfEdges = ints(kfEdges); D.mpStart = ints(mpStart); D.mpEdges = ints(mpEdges);
    D.pairStart = ints(pairStart); D.pairEdges = ints(pairEdges); D.pairCol = ints(pairCol); D.pairMp = ints(pairMp); D.mpPairStart = ints(mpPairStart);
    D.kfPairStart = ints(kfPairStart); D.kfPairs = ints(kfPairs);
    D.rowFirst = ints(P.rowFirst); D.rowOff = ints(P.rowOff); D.colStart = ints(P.colStart); D.colRows = ints(P.colRows);
    D.blkDiag = ints(blkDiag); D.chunkStart = ints(chunkStart); D.chunkEnd = ints(chunkEnd); D.blkChunkStart = ints(blkChunkStart);
    D.ct = (const int2*)A.take(ct.data(), sizeof(int2) * nCt);
    D.pose = (double*)A.take(pose.data(), sizeof(double) * 7 * nKF); D.pt = (double*)A.take(pt.data(), sizeof(double) * 3 * nMP);
    if (rig) D.rig = (const Rig*)A.take(rig, sizeof(Rig));
    D.poseT = (double*)A.take(nullptr, sizeof(double) * 7 * nKF); D.ptT = (double*)A.take(nullptr, sizeof(double) * 3 * nMP);
    D.E = (double*)A.take(nullptr, sizeof(double) * GBA_EDGE * nE);
    D.Hpp = (double*)A.take(nullptr, sizeof(double) * 36 * n); D.bp = (double*)A.take(nullptr, sizeof(double) * 6 * n);
    D.Hll = (double*)A.take(nullptr, sizeof(double) * 9 * nMP); D.bl = (double*)A.take(nullptr, sizeof(double) * 3 * nMP);
    D.Dinv = (double*)A.take(nullptr, sizeof(double) * 9 * nMP); D.xl = (double*)A.take(nullptr, sizeof(double) * 3 * nMP);
    D.Hpl = (double*)A.take(nullptr, sizeof(double) * 18 * nPairs); D.HplD = (double*)A.take(nullptr, sizeof(double) * 18 * nPairs);
    D.g = (double*)A.take(nullptr, sizeof(double) * 6 * nPairs);
    D.part = (double*)A.take(nullptr, sizeof(double) * 36 * (size_t)nChunks);
    D.H = (double*)A.take(nullptr, sizeof(double) * 36 * (size_t)nBlocks); D.L = (double*)A.take(nullptr, sizeof(double) * 36 * (size_t)nBlocks);
    D.b = (double*)A.take(nullptr, sizeof(double) * 6 * n); D.y = (double*)A.take(nullptr, sizeof(double) * 6 * n);
    D.x = (double*)A.take(nullptr, sizeof(double) * 6 * n); D.d = (double*)A.take(nullptr, sizeof(double) * 6 * n);
    D.chiE = (double*)A.take(nullptr, sizeof(double) * nE);
    D.lm = (LmControl*)A.take(nullptr, sizeof(LmControl)); D.chi2 = (double*)A.take(nullptr, sizeof(double) * 2);
    D.lmi = (int*)A.take(nullptr, sizeof(int) * 8);
  };
  carve();   // (dry: sizes)
  char *arena = nullptr, *stage = nullptr;
  { const int rc = grow(o->globalBA, A.uploadBytes() + A.deviceBytes(), &arena); if (rc != MORB_OK) return rc; }
  { const int rc = grow(o->stage, A.uploadBytes(), &stage); if (rc != MORB_OK) return rc; }
  A.bind(arena, stage);
  carve();
  if (!A.ok()) { set_error("the two carve passes of BundleAdjustment differ"); return MORB_ERR_HIP; }
  int *hostw = nullptr, *hostwDev = nullptr;
  MORB_REQUIRE(morb_optimizer_lm_words(o, &hostw, &hostwDev) == MORB_OK, MORB_ERR_HIP, "cannot map the LM state words");
  D.lmHost = hostwDev;
  const volatile uint8_t* userStop = stopFlag;
  auto forwardStop = [&]() { if (userStop && *userStop) __atomic_store_n(hostw + 2, 1, __ATOMIC_RELEASE); };   // optimizer.setForceStopFlag(pbStopFlag) (:78)
  reset_lm_words(hostw, 2, hostw + 2);
  forwardStop();
  MORB_HIP_CHECK(hipMemcpyAsync(arena, stage, A.uploadBytes(), hipMemcpyHostToDevice, st));   // the one upload
  // the workspace is reused from call to call: what the first kernels expect to find zero is cleared
  MORB_HIP_CHECK(hipMemsetAsync(D.lmi, 0, sizeof(int) * 8, st));
  MORB_HIP_CHECK(hipMemsetAsync(D.lm, 0, sizeof(LmControl), st));
  MORB_HIP_CHECK(hipMemsetAsync(D.x, 0, sizeof(double) * 6 * n, st));        // the step before the first solve
  MORB_HIP_CHECK(hipMemsetAsync(D.xl, 0, sizeof(double) * 3 * nMP, st));

  const int edgeBlocks = div_up(nE, GBA_NT);
  const size_t asmItems = (size_t)n * 42 + (size_t)nMP * 12 + (size_t)nPairs * 18;
  const size_t finItems = (size_t)nBlocks * 36 + (size_t)n * 6;
  auto blocks = [](size_t items) { return dim3((unsigned)((items + GBA_NT - 1) / GBA_NT)); };
  hipLaunchKernelGGL(k_gba_errors, dim3(edgeBlocks), dim3(GBA_NT), 0, st, D, 0);   // computeActiveErrors
  hipLaunchKernelGGL(k_gba_decide, dim3(1), dim3(GBA_NT), 0, st, D, 1);
  MORB_HIP_CHECK(hipGetLastError());
  // a slot is one trial: at most nIterations iterations of 10 trials
  const int q = lm_slot_queue(10 * nIterations, hostw + 0, hostw + 1, [&](int) {
    if (rig) hipLaunchKernelGGL(k_gba_linearize<true>, dim3(edgeBlocks), dim3(GBA_NT), 0, st, D);   // (the first three run only behind an accepted trial)
    else hipLaunchKernelGGL(k_gba_linearize<false>, dim3(edgeBlocks), dim3(GBA_NT), 0, st, D);
    hipLaunchKernelGGL(k_gba_assemble, blocks(asmItems), dim3(GBA_NT), 0, st, D);
    hipLaunchKernelGGL(k_gba_maxdiag, dim3(1), dim3(GBA_NT), 0, st, D);                             // (behind the first assembly only)
    hipLaunchKernelGGL(k_gba_dinv, dim3(div_up(nMP + nPairs, GBA_NT)), dim3(GBA_NT), 0, st, D);
    hipLaunchKernelGGL(k_gba_schur, blocks((size_t)nChunks * 36), dim3(GBA_NT), 0, st, D);
    hipLaunchKernelGGL(k_gba_schur_finish, blocks(finItems), dim3(GBA_NT), 0, st, D);
    hipLaunchKernelGGL(k_gba_factor, dim3(1), dim3(GBA_NT), 0, st, D);
    hipLaunchKernelGGL(k_gba_backsub, dim3(1), dim3(GBA_NT), 0, st, D);
    hipLaunchKernelGGL(k_gba_points, dim3(div_up(nMP, GBA_NT)), dim3(GBA_NT), 0, st, D);
    hipLaunchKernelGGL(k_gba_errors, dim3(edgeBlocks), dim3(GBA_NT), 0, st, D, 1);
    hipLaunchKernelGGL(k_gba_decide, dim3(1), dim3(GBA_NT), 0, st, D, 0);
    if (hipGetLastError() != hipSuccess) { set_error("BundleAdjustment: a trial's launch failed"); return (int)MORB_ERR_HIP; }
    return (int)MORB_OK;
  }, [&]() { return stream_look(st, "BundleAdjustment"); }, forwardStop);
  if (q < 0) return MORB_ERR_HIP;
  int hi[8];
  double c2[2];
  MORB_HIP_CHECK(hipMemcpyAsync(hi, D.lmi, sizeof hi, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipMemcpyAsync(c2, D.chi2, sizeof c2, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipMemcpyAsync(pose.data(), D.pose, sizeof(double) * 7 * nKF, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipMemcpyAsync(pt.data(), D.pt, sizeof(double) * 3 * nMP, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipStreamSynchronize(st));   // (also drains a queue that ran out of slots before the words are reset again)
  // (:276-361) the keyframes of the system and the points that carry an edge; everything else keeps its bytes
  for (int v = 0; v < nKF; ++v) if (P.col[v] >= 0) for (int k = 0; k < 7; ++k) kfPose[7 * v + k] = (float)pose[(size_t)7 * v + k];
  for (int m = 0; m < nMP; ++m) if (mpStart[m + 1] > mpStart[m]) for (int k = 0; k < 3; ++k) mpPos[3 * m + k] = (float)pt[(size_t)3 * m + k];
  stats4[0] = hi[LMW_ITS]; stats4[1] = hi[LMW_TRIALS]; stats4[2] = n; stats4[3] = nBlocks;
  chi2[0] = c2[0]; chi2[1] = c2[1];
  return MORB_OK;
}

}  // namespace

extern "C" int morb_bundle_adjustment(morb_optimizer* o, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos, int nE,
                                      const int* eKF, const int* eMP, const float* eObs, const float* eInvSigma2, float fx, float fy, float cx,
                                      float cy, float bf, int nIterations, int bRobust, const uint8_t* stopFlag, int* stats4, double* chi2) {
  return gba_run(o, nKF, kfPose, kfFixed, nMP, mpPos, nE, eKF, eMP, eObs, eInvSigma2, Cam{fx, fy, cx, cy, bf}, nullptr, nIterations, bRobust,
                 stopFlag, stats4, chi2);
}

extern "C" int morb_bundle_adjustment_fisheye(morb_optimizer* o, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos, int nE,
                                              const int* eKF, const int* eMP, const float* eObs2, const uint8_t* eRight, const float* eInvSigma2,
                                              const float* camL8, const float* camR8, const float* Trl7, int nIterations, int bRobust,
                                              const uint8_t* stopFlag, int* stats4, double* chi2) {
  MORB_REQUIRE(eObs2 && eRight && camL8 && camR8 && Trl7, MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nE > 0, MORB_ERR_INVALID, "empty problem");
  for (int k = 0; k < 8; ++k) MORB_REQUIRE(std::isfinite(camL8[k]) && std::isfinite(camR8[k]), MORB_ERR_INVALID, "a non-finite camera");
  for (int k = 0; k < 7; ++k) MORB_REQUIRE(std::isfinite(Trl7[k]), MORB_ERR_INVALID, "a non-finite Trl");
  // the edge kind travels in the third slot of the observation: -2 = EdgeSE3ProjectXYZ on the left camera, -3 = EdgeSE3ProjectXYZToBody
  std::vector<float> obs3((size_t)nE * 3);
  for (int e = 0; e < nE; ++e) { obs3[3 * e] = eObs2[2 * e]; obs3[3 * e + 1] = eObs2[2 * e + 1]; obs3[3 * e + 2] = eRight[e] ? -3.0f : -2.0f; }
  const Rig rig = make_rig(camL8, camR8, Trl7);
  return gba_run(o, nKF, kfPose, kfFixed, nMP, mpPos, nE, eKF, eMP, obs3.data(), eInvSigma2, Cam{0.f, 0.f, 0.f, 0.f, 0.f}, &rig, nIterations,
                 bRobust, stopFlag, stats4, chi2);
}
