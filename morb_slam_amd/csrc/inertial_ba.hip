// LocalInertialBA (reference src/Optimizer.cc:2324-2897) for MI355X (gfx950), on the handle of optimizer.hip and the device helpers of
// inertial_device.h: the temporal window of keyframes with 15-dof states, the points they see behind a Schur complement, the chain of
// inertial / random-walk edges.  g2o Levenberg-Marquardt semantics (optimization_algorithm_levenberg.cpp:61-194, block_solver.hpp) with
// the control flow on the device, like the grid mode of LocalBundleAdjustment (local_ba.hip): the last workgroup of k_iba_errors takes a
// trial's accept / reject decision (iba_lm_decide); the host queues trial slots one ahead and watches a mapped word (iba_lm_loop).
// MergeInertialBA (:3853-4389), the welding bundle adjustment of an inertial map merge, is the same graph with another plan (IbaPlan) and
// with keyframes that are free in the pose only: every free keyframe owns 15 or 6 columns of the reduced system (off / wid / colOff), two
// temporal chains are nothing but link indices, and the caller's *pbStopFlag reaches the decision through a mapped word.
// One launch per phase over the whole chip:
//   k_iba_errors   computeActiveErrors + activeRobustChi2 (one thread per visual edge / per inertial link)
//   k_iba_points   per point: Hll, bl                      k_iba_kf   per 64-edge chunk of a keyframe: Hpp, bp (wave sums), Hpl
//   k_iba_links    inertial + random-walk edges into the dense 15 N x 15 N system
//   k_iba_pack_w / k_iba_pack_wd + k_schur_mfma + k_iba_schur_finish   Schur complement of the points on the FP64 matrix cores
//   k_iba_solve_lds / k_iba_solve_blocked   one workgroup: dense LDL^T (dense_ldlt.h), in LDS or in global memory by the window's size
//   k_iba_update   back-substitution of the points, oplus of all vertices
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "common.h"
#include "internal_abi.h"
#include "ba_host.h"
#include "dense_ldlt.h"
#include "schur_mfma.h"
#include "wave.h"
#include "inertial_device.h"

using namespace morb;

namespace {

struct IbaDev {
  int nKF, nMP, nE, nI, P, nChunks;
  const int *eKF, *eMP;
  const float *eObs, *eInfo;
  const int *ptStart, *ptEdges;                 // CSR by point
  const int *kfEdges, *chunkKF, *chunkStart, *chunkEnd;   // edges of free keyframes in chunks of <= 64
  double* kfPart; int* kfTicket;                          // per-chunk partial sums of k_iba_kf (27 each), arrival counter per keyframe
  const int* linkOrder;                                   // inertial links sorted by colour: links of one colour share no keyframe
  const int* col;                               // [nKF] pose-block index of a free keyframe (the MFMA Schur operands' columns 6 c + r) or -1
  const int* off;                               // [nKF] first column of a free keyframe in the reduced system (15 or 6 columns wide) or -1
  const int* wid;                               // [nKF] 15: pose, velocity, biases | 6: free in the pose only | 0: fixed
  const int* colOff;                            // [nFree] off[] by pose-block index (the inverse of col, for k_iba_schur_finish)
  int nFree;                                    // free keyframes of either width: the Schur operands have M = 6 nFree + 1 columns
  const int *iKF1, *iKF2;
  const morb_imu_preintegrated* iPre;
  const uint8_t* iRobust;
  const uint8_t* mpClose;
  const uint8_t* eRight;                        // fisheye rig: edge on the right camera (NULL: pinhole)
  double* S;                                    // [nKF][33]: Rwb twb v bg ba | Rcw tcw
  double* pts;                                  // [nMP][3]
  double *vErr, *iErr, *gErr, *aErr;            // errors of the last computeActiveErrors
  double *InfoI, *InfoG, *InfoA;
  double *H, *b, *Hll, *Hpl, *Hs, *bs, *x;      // b, x: P + 3 nMP
  double* scal;                                 // [0] robust chi2 of the last k_iba_errors, [2] solve ok
  double *partChi, *partScale; int nbUpdate;    // per-block partial sums of k_iba_errors / k_iba_update (added up in block order)
  // Schur complement on the FP64 matrix cores (schur_mfma.h): dense K-major operands (columns 6 c + r of the pose parts, plus
  // the right-hand-side column 6 nFree), partial products, block directory
  double *sW, *sWD, *sPart;
  const int2* sBlocks;
  const int* sBlkIndex;
  int sMp, sNb, sNblk, sNsplit;
  // device-side LM control (see local_ba.hip, grid mode): the loop state, its mirror in mapped host memory, the backups
  double* lmd;                                  // IBA_LMD_*: currentChi, lambda, ni, iniChi, chi2 of the last evaluated trial
  int* lmi;                                     // IBA_LM_*
  int* lmHost;                                  // [0] decided trials, [1] done
  double *Sbk, *ptsBk;                          // state / points before the trial
  double* pnlG;                                 // panel copies of the global-memory LDL^T when they do not fit LDS
  int nS, nPts;
  // the plan (LocalInertialBA | MergeInertialBA): iterations, the erase rule; robust / scaled links travel per link (iRobust, InfoI)
  int optIt, eraseChi2Only;
  const int* stopWord;                          // the caller's *pbStopFlag as the host loop forwards it (mapped host word), or NULL
  CamGeom g;
};
enum { IBA_LM_ITER, IBA_LM_QMAX, IBA_LM_NBAD, IBA_LM_ITS, IBA_LM_TRIALS, IBA_LM_DONE, IBA_LM_NEEDBUILD, IBA_LM_REJECTED, IBA_LM_TICKET };
enum { IBA_LMD_CHI, IBA_LMD_LAMBDA, IBA_LMD_NI, IBA_LMD_INICHI, IBA_LMD_LASTCHI };
__device__ __forceinline__ bool iba_done(const IbaDev& D) { return D.lmi[IBA_LM_DONE] != 0; }
__device__ __forceinline__ bool iba_no_build(const IbaDev& D) { return D.lmi[IBA_LM_DONE] != 0 || D.lmi[IBA_LM_NEEDBUILD] == 0; }
__device__ __forceinline__ bool iba_stop_requested(const IbaDev& D) {   // (as lm_stop_requested of local_ba.hip)
  return D.stopWord && __hip_atomic_load(D.stopWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
}
__device__ __forceinline__ void iba_load(const CamGeom& g, const double* s, VIState& V) {
  for (int k = 0; k < 9; ++k) { V.Rwb[k] = s[k]; V.Rcw[k] = s[21 + k]; }
  for (int k = 0; k < 3; ++k) { V.twb[k] = s[9 + k]; V.v[k] = s[12 + k]; V.bg[k] = s[15 + k]; V.ba[k] = s[18 + k]; V.tcw[k] = s[30 + k]; }
  if (g.rig) refresh_camera(g, V);   // the right camera's pose is derived, not stored
}
__device__ __forceinline__ void iba_store(const VIState& V, double* s) {
  for (int k = 0; k < 9; ++k) { s[k] = V.Rwb[k]; s[21 + k] = V.Rcw[k]; }
  for (int k = 0; k < 3; ++k) { s[9 + k] = V.twb[k]; s[12 + k] = V.v[k]; s[15 + k] = V.bg[k]; s[18 + k] = V.ba[k]; s[30 + k] = V.tcw[k]; }
}
__device__ __forceinline__ double huber_rho(double delta, double e2) {   // rho(e2)
  return e2 <= delta * delta ? e2 : 2 * sqrt(e2) * delta - delta * delta;
}
// Sum over the block, in a fixed order (DPP tree per wave, then the waves in turn): thread 0 holds it.  The blocks' sums are stored one per
// block and added up in block order by whoever consumes them — a floating-point atomicAdd per block would make the chi2, through rho and
// lambda every later iterate, depend on the order in which the blocks happen to finish (seen as last-bit differences between two runs).
__device__ __forceinline__ double block_sum(double v) {
  __shared__ double red[16];
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  if (lane == 0) red[wv] = v;
  __syncthreads();
  double s = 0;
  if (threadIdx.x == 0) for (int w = 0; w < nw; ++w) s += red[w];
  __syncthreads();
  return s;
}
// The partial sums of n workgroups added up by one full wave, always in the same order (lane k takes partials k, k + 64, ...; then the DPP
// tree): every lane returns the total.  The partials were written by other workgroups: agent-scope loads.
__device__ __forceinline__ double ordered_sum_wave(const double* part, int n) {
  double s = 0;
  for (int k = threadIdx.x & 63; k < n; k += 64)
    s += __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const unsigned long long*>(part + k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  return wave_sum(s);
}
__device__ __forceinline__ double iba_vis_chi2(const IbaDev& D, int e) {
  const double info = (double)D.eInfo[e];
  const double* er = D.vErr + 3 * (size_t)e;
  return er[0] * info * er[0] + er[1] * info * er[1] + er[2] * info * er[2];   // mono: er[2] = 0
}
__device__ __forceinline__ double iba_quad(const double* e, const double* Om, int n) {
  double s = 0;
  for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) s += e[r] * Om[r * n + c] * e[c];
  return s;
}

__global__ void k_iba_setup_kf(IbaDev D, const float* __restrict__ kfState) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= D.nKF) return;
  VIState V;
  load_state(D.g, kfState + 21 * k, V);
  iba_store(V, D.S + 33 * (size_t)k);
}
__global__ void k_iba_setup_pts(IbaDev D, const float* __restrict__ mpPos) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < D.nPts) D.pts[k] = (double)mpPos[k];
}
// informations of the inertial links: one workgroup per link, the 9 x 9 work arrays in LDS (one thread computes)
__global__ __launch_bounds__(64) void k_iba_setup_links(IbaDev D, const float* __restrict__ infoScale) {
  __shared__ double C9[81], M[162], V[162], Inf[81];
  const int i = blockIdx.x;
  if (threadIdx.x == 0) {
    const morb_imu_preintegrated& P = D.iPre[i];
    for (int r = 0; r < 9; ++r) for (int c = 0; c < 9; ++c) C9[r * 9 + c] = (double)P.C[r * 15 + c];
    if (invert_n(C9, 9, Inf, M)) {
      for (int r = 0; r < 9; ++r) for (int c = r + 1; c < 9; ++c) { const double s = (Inf[r * 9 + c] + Inf[c * 9 + r]) / 2; Inf[r * 9 + c] = s; Inf[c * 9 + r] = s; }
      clamp_eigenvalues(Inf, 9, 1e-12, M, V);
    } else for (int k = 0; k < 81; ++k) Inf[k] = 0;
    double Cg[9], Ca[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { Cg[r * 3 + c] = P.C[(9 + r) * 15 + 9 + c]; Ca[r * 3 + c] = P.C[(12 + r) * 15 + 12 + c]; }
    if (!invert_n(Cg, 3, D.InfoG + (size_t)i * 9, M)) for (int k = 0; k < 9; ++k) D.InfoG[(size_t)i * 9 + k] = 0;
    if (!invert_n(Ca, 3, D.InfoA + (size_t)i * 9, M)) for (int k = 0; k < 9; ++k) D.InfoA[(size_t)i * 9 + k] = 0;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 81; k += 64) D.InfoI[(size_t)i * 81 + k] = Inf[k] * (double)infoScale[i];
}

// computeActiveErrors + activeRobustChi2 -> scal[0] (the last workgroup to finish adds the blocks' partial sums up in block order)
__device__ void iba_lm_decide(const IbaDev& D, double trialChi2, double gain);
// mode 0: computeActiveErrors + activeRobustChi2.  mode 1 (a trial under device-side LM control):
// returns at once when the solve has finished; the last workgroup to finish takes the trial's accept / reject decision.
__global__ __launch_bounds__(256) void k_iba_errors(IbaDev D, int mode) {
  if (mode == 1 && iba_done(D)) return;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const double deltaMono = (double)(float)sqrt(5.991), deltaStereo = (double)(float)sqrt(7.815), deltaI = sqrt(16.92);
  double c = 0;
  if (t < D.nE) {
    VIState V;
    iba_load(D.g, D.S + 33 * (size_t)D.eKF[t], V);
    const float* o = D.eObs + 3 * (size_t)t;
    const bool st = !D.g.rig && !(o[2] < 0);
    const double* Xp = D.pts + 3 * (size_t)D.eMP[t];
    const double X[3] = {Xp[0], Xp[1], Xp[2]};
    double err[3], Xc[3];
    const double chi = vis_error(D.g, V, X, o, st, (double)D.eInfo[t], err, Xc, D.eRight && D.eRight[t] ? 1 : 0);
    for (int k = 0; k < 3; ++k) D.vErr[3 * (size_t)t + k] = err[k];
    c = huber_rho(st ? deltaStereo : deltaMono, chi);
  } else if (t - D.nE < D.nI) {
    const int i = t - D.nE;
    VIState V1, V2;
    iba_load(D.g, D.S + 33 * (size_t)D.iKF1[i], V1);
    iba_load(D.g, D.S + 33 * (size_t)D.iKF2[i], V2);
    double err[9];
    inertial_edge(D.iPre[i], V1, V2, nullptr, true, err, nullptr);
    double ge[3], ae[3];
    for (int k = 0; k < 9; ++k) D.iErr[9 * (size_t)i + k] = err[k];
    for (int k = 0; k < 3; ++k) { ge[k] = V2.bg[k] - V1.bg[k]; ae[k] = V2.ba[k] - V1.ba[k]; D.gErr[3 * i + k] = ge[k]; D.aErr[3 * i + k] = ae[k]; }
    const double ci = iba_quad(err, D.InfoI + (size_t)i * 81, 9);
    c = (D.iRobust[i] ? huber_rho(deltaI, ci) : ci) + iba_quad(ge, D.InfoG + (size_t)i * 9, 3) + iba_quad(ae, D.InfoA + (size_t)i * 9, 3);
  }
  const double bs = block_sum(c);
  __shared__ int isLast;
  if (threadIdx.x == 0) {   // hand-off without __threadfence() (an L2 write-back per workgroup on this chip): write-through store, wait, relaxed ticket
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(D.partChi + blockIdx.x), __builtin_bit_cast(unsigned long long, bs), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    isLast = __hip_atomic_fetch_add(&D.lmi[IBA_LM_TICKET], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!isLast || threadIdx.x >= 64) return;   // the last workgroup's first wave adds the partials up
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (ordered_sum_wave reads every handed-off word at agent scope)
  const double chi2 = ordered_sum_wave(D.partChi, (int)gridDim.x);
  const double gain = mode == 1 ? ordered_sum_wave(D.partScale, D.nbUpdate) : 0.0;   // k_iba_update's blocks
  if (threadIdx.x != 0) return;
  D.lmi[IBA_LM_TICKET] = 0;
  D.scal[0] = chi2;
  if (mode == 1) iba_lm_decide(D, chi2, gain);
}
// optimization_algorithm_levenberg.cpp:99-169 with ORB-SLAM's stop rule, as local_inertial_ba_impl's host loop ran it: rho from
// the trial's chi2, the linear-model gain (the sum of k_iba_update's per-block partials) and the solver's flag (scal[2]).  One thread.
__device__ void iba_lm_decide(const IbaDev& D, double trialChi2, double gain) {
  const double s0 = trialChi2;
  const double s1 = gain;
  const bool ok2 = D.scal[2] != 0.0;
  double currentChi = D.lmd[IBA_LMD_CHI], lambda = D.lmd[IBA_LMD_LAMBDA], ni = D.lmd[IBA_LMD_NI];
  const double iniChi = D.lmd[IBA_LMD_INICHI];
  int iter = D.lmi[IBA_LM_ITER], qmax = D.lmi[IBA_LM_QMAX], nBad = D.lmi[IBA_LM_NBAD], its = D.lmi[IBA_LM_ITS];
  double tempChi = s0;
  if (!ok2) tempChi = 1.7976931348623157e308;
  const double rho = (currentChi - tempChi) / (s1 + 1e-3);
  const bool accept = rho > 0 && isfinite(tempChi);
  if (accept) {
    double alpha = 1. - pow((2 * rho - 1), 3);
    alpha = fmin(alpha, 2. / 3.);
    lambda *= fmax(1. / 3., alpha);
    ni = 2;
    currentChi = tempChi;
  } else {
    lambda *= ni;
    ni *= 2;
  }
  ++qmax;
  const int trials = D.lmi[IBA_LM_TRIALS] + 1;
  const bool stop = iba_stop_requested(D);
  int done = 0, needBuild = 0;
  if (!(rho < 0 && qmax < 10 && !stop)) {   // the trial loop ends
    // (a NaN rho — NaN errors — leaves the loop with the trial rejected: the host loop went on from the restored state; here the
    // solve ends, the stored errors belong to the rejected state)
    bool fin = (qmax == 10 || rho == 0 || !(rho == rho));
    if (!fin) { if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0; fin = nBad >= 3; }
    if (!fin) { ++iter; fin = iter >= D.optIt || stop; }
    if (fin) done = 1;
    else { ++its; qmax = 0; needBuild = 1; D.lmd[IBA_LMD_INICHI] = currentChi; }
  }
  D.lmd[IBA_LMD_CHI] = currentChi; D.lmd[IBA_LMD_LAMBDA] = lambda; D.lmd[IBA_LMD_NI] = ni; D.lmd[IBA_LMD_LASTCHI] = s0;
  D.lmi[IBA_LM_ITER] = iter; D.lmi[IBA_LM_QMAX] = qmax; D.lmi[IBA_LM_NBAD] = nBad; D.lmi[IBA_LM_ITS] = its; D.lmi[IBA_LM_TRIALS] = trials;
  D.lmi[IBA_LM_DONE] = done; D.lmi[IBA_LM_NEEDBUILD] = needBuild; D.lmi[IBA_LM_REJECTED] = accept ? 0 : 1;
  __hip_atomic_store(D.lmHost + 1, done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(D.lmHost + 0, trials, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// after the last slot: a rejected last trial is undone
__global__ __launch_bounds__(256) void k_iba_end(IbaDev D) {
  if (!D.lmi[IBA_LM_REJECTED]) return;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < D.nS) D.S[t] = D.Sbk[t];
  if (t < D.nPts) D.pts[t] = D.ptsBk[t];
}
__global__ void k_iba_lm_init(IbaDev D, double chi, double lambda0) {
  D.lmd[IBA_LMD_CHI] = chi; D.lmd[IBA_LMD_LAMBDA] = lambda0; D.lmd[IBA_LMD_NI] = 2; D.lmd[IBA_LMD_INICHI] = chi; D.lmd[IBA_LMD_LASTCHI] = chi;
  for (int k = 0; k < 16; ++k) D.lmi[k] = 0;
  const bool stop = iba_stop_requested(D);   // raised since the entry's own test: no iteration runs
  D.lmi[IBA_LM_ITS] = stop ? 0 : 1; D.lmi[IBA_LM_DONE] = stop ? 1 : 0; D.lmi[IBA_LM_NEEDBUILD] = 1;
  D.scal[0] = 0.0; D.scal[1] = 0.0;
  if (stop) __hip_atomic_store(D.lmHost + 1, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// point side of buildSystem: Hll, bl (one thread per point over its edges, no atomics)
// (the launch starts with k_iba_begin's work — backup / restore, clearing the accumulators — on as many threads as that needs)
__device__ __forceinline__ void iba_begin_part(const IbaDev& D, int t) {
  const bool restore = D.lmi[IBA_LM_REJECTED] != 0;
  if (restore) {
    if (t < D.nS) D.S[t] = D.Sbk[t];
    if (t < D.nPts) D.pts[t] = D.ptsBk[t];
  } else {
    if (t < D.nS) D.Sbk[t] = D.S[t];
    if (t < D.nPts) D.ptsBk[t] = D.pts[t];
  }
  if (D.lmi[IBA_LM_NEEDBUILD]) {
    if (t < D.P * D.P) D.H[t] = 0.0;
    if (t < D.P) D.b[t] = 0.0;
    if (t < 18 * D.nE) D.Hpl[t] = 0.0;
  }
}
constexpr int IBA_PT_LANES = 8;   // lanes per point in k_iba_points
__global__ __launch_bounds__(256) void k_iba_points(IbaDev D) {
  __shared__ double sPt[256 * 12];
  if (iba_done(D)) return;
  iba_begin_part(D, blockIdx.x * 256 + threadIdx.x);
  if (D.lmi[IBA_LM_NEEDBUILD] == 0) return;   // (a rebuild follows an accepted trial: nothing was restored, the points read below are current)
  // EIGHT lanes per point, one edge each and chunk by chunk; the twelve contributions of an edge go to the wave's LDS slice and the group's first lane
  // adds them up in edge order: the sums of the one-thread-per-point walk this replaces, bit for bit (as in LocalBundleAdjustment's k_g_build)
  const int g = threadIdx.x / IBA_PT_LANES, sub = threadIdx.x % IBA_PT_LANES;
  const int l = blockIdx.x * (256 / IBA_PT_LANES) + g;
  const bool live = l < D.nMP;
  double* slot = sPt + (size_t)g * IBA_PT_LANES * 12;
  const double deltaMono = (double)(float)sqrt(5.991), deltaStereo = (double)(float)sqrt(7.815);
  double Hl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
  const size_t lp = live ? (size_t)l : 0;
  const double X[3] = {D.pts[3 * lp], D.pts[3 * lp + 1], D.pts[3 * lp + 2]};
  const int k0 = live ? D.ptStart[l] : 0, k1 = live ? D.ptStart[l + 1] : 0;
  for (int kb = k0; kb < k1; kb += IBA_PT_LANES) {
    const int k = kb + sub;
    double c12[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) c12[q] = 0;
    if (k < k1) {
      const int e = D.ptEdges[k];
      VIState V;
      iba_load(D.g, D.S + 33 * (size_t)D.eKF[e], V);
      const int cam = D.eRight && D.eRight[e] ? 1 : 0;
      const double* Rc = cam ? V.Rcw1 : V.Rcw;
      const double* tc = cam ? V.tcw1 : V.tcw;
      const float* o = D.eObs + 3 * (size_t)e;
      const bool st = !D.g.rig && !(o[2] < 0);
      const double info = (double)D.eInfo[e];
      const double w = huber_w(st ? deltaStereo : deltaMono, iba_vis_chi2(D, e));
      double Xc[3];
      for (int r = 0; r < 3; ++r) Xc[r] = Rc[r * 3] * X[0] + Rc[r * 3 + 1] * X[1] + Rc[r * 3 + 2] * X[2] + tc[r];
      // -proj_jac * Rcw (G2oTypes.cc:334-415)
      double pj[9];
      cam_project_jac(D.g, Xc, cam, pj);
      pj[6] = pj[7] = pj[8] = 0;
      if (st) { pj[6] = pj[0]; pj[7] = pj[1]; pj[8] = pj[2] + D.g.bf * (1.0 / (Xc[2] * Xc[2])); }
      double Jl[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Jl[r * 3 + c] = -(pj[r * 3] * Rc[c] + pj[r * 3 + 1] * Rc[3 + c] + pj[r * 3 + 2] * Rc[6 + c]);
      const double* er = D.vErr + 3 * (size_t)e;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double sm = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) sm += Jl[i * 3 + r] * info * er[i];
        c12[9 + r] = w * sm;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double h = 0;
#pragma unroll
          for (int i = 0; i < 3; ++i) h += Jl[i * 3 + r] * (w * info) * Jl[i * 3 + c];
          c12[r * 3 + c] = h;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) slot[sub * 12 + q] = c12[q];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (sub == 0) {
      const int cnt = k1 - kb < IBA_PT_LANES ? k1 - kb : IBA_PT_LANES;
      for (int j = 0; j < cnt; ++j) {
#pragma unroll
        for (int q = 0; q < 9; ++q) Hl[q] += slot[j * 12 + q];
#pragma unroll
        for (int q = 0; q < 3; ++q) bl[q] -= slot[j * 12 + 9 + q];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   // (the slice is rewritten by the next chunk)
  }
  if (!live || sub != 0) return;
  for (int k = 0; k < 9; ++k) D.Hll[(size_t)l * 9 + k] = Hl[k];
  for (int k = 0; k < 3; ++k) D.b[D.P + 3 * (size_t)l + k] = bl[k];
}
// keyframe side: one wave per chunk of <= 64 edges of one optimizable keyframe
__global__ __launch_bounds__(256) void k_iba_kf(IbaDev D) {
  if (iba_no_build(D)) return;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= D.nChunks) return;
  const double deltaMono = (double)(float)sqrt(5.991), deltaStereo = (double)(float)sqrt(7.815);
  const int kf = D.chunkKF[c];
  VIState V;
  iba_load(D.g, D.S + 33 * (size_t)kf, V);
  double acc[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) acc[k] = 0;
  const int k = D.chunkStart[c] + lane;
  if (k < D.chunkEnd[c]) {
    const int e = D.kfEdges[k];
    const float* o = D.eObs + 3 * (size_t)e;
    const bool st = !D.g.rig && !(o[2] < 0);
    const int cam = D.eRight && D.eRight[e] ? 1 : 0;
    double Rc[9], tc[3];   // (element-wise selects: a pointer chosen between two members of V sends V to scratch memory)
#pragma unroll
    for (int r = 0; r < 9; ++r) Rc[r] = cam ? V.Rcw1[r] : V.Rcw[r];
#pragma unroll
    for (int r = 0; r < 3; ++r) tc[r] = cam ? V.tcw1[r] : V.tcw[r];
    const double info = (double)D.eInfo[e];
    const double w = huber_w(st ? deltaStereo : deltaMono, iba_vis_chi2(D, e));
    const double* Xp = D.pts + 3 * (size_t)D.eMP[e];
    const double X[3] = {Xp[0], Xp[1], Xp[2]};
    double Xc[3], Jp[18], Jl[9];
    mul3v(Rc, X, Xc);
    for (int r = 0; r < 3; ++r) Xc[r] += tc[r];
    vis_jacobian(D.g, Xc, st, Jp, cam);
    double pj[9];
    cam_project_jac(D.g, Xc, cam, pj);
    pj[6] = pj[7] = pj[8] = 0;
    if (st) { pj[6] = pj[0]; pj[7] = pj[1]; pj[8] = pj[2] + D.g.bf * (1.0 / (Xc[2] * Xc[2])); }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) Jl[r * 3 + cc] = -(pj[r * 3] * Rc[cc] + pj[r * 3 + 1] * Rc[3 + cc] + pj[r * 3 + 2] * Rc[6 + cc]);
    const double* er = D.vErr + 3 * (size_t)e;
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double sm = 0;
#pragma unroll
      for (int i = 0; i < 3; ++i) sm += Jp[i * 6 + r] * info * er[i];
      acc[21 + r] = -w * sm;
#pragma unroll
      for (int cc = r; cc < 6; ++cc) {
        double h = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) h += Jp[i * 6 + r] * (w * info) * Jp[i * 6 + cc];
        acc[q++] = h;
      }
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) {
        double h = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) h += Jp[i * 6 + r] * (w * info) * Jl[i * 3 + cc];
        D.Hpl[(size_t)e * 18 + r * 3 + cc] = h;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 27; ++q) acc[q] = wave_sum(acc[q]);
  // A keyframe's chunks are added up in chunk order by whichever of them finishes last (floating-point atomics would add them in
  // arrival order: the Hessian, and with it every iterate, would differ in the last bits from run to run).  Nothing else has touched the
  // keyframe's pose block yet — the links are launched afterwards — so the sum is stored with plain read-modify-writes.
  int first = c, end = c + 1, last = 0;
  if (lane == 0) {   // (hand-off as in k_iba_errors: write-through stores, wait, relaxed ticket; the last arriver reads at agent scope)
#pragma unroll
    for (int q = 0; q < 27; ++q)
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(D.kfPart + (size_t)c * 27 + q), __builtin_bit_cast(unsigned long long, acc[q]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (first > 0 && D.chunkKF[first - 1] == kf) --first;
    while (end < D.nChunks && D.chunkKF[end] == kf) ++end;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = __hip_atomic_fetch_add(&D.kfTicket[kf], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == end - first - 1;
  }
  last = __builtin_amdgcn_readfirstlane(last);
  if (!last) return;
  first = __builtin_amdgcn_readfirstlane(first); end = __builtin_amdgcn_readfirstlane(end);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane == 0) D.kfTicket[kf] = 0;
  if (lane < 27) {
    double sum = 0;
    const double* part = D.kfPart + lane;
    for (int j = first; j < end; ++j)
      sum += __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const unsigned long long*>(part + (size_t)j * 27), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const int o = D.off[kf];
    if (lane >= 21) D.b[o + lane - 21] += sum;
    else {
      int r = 0, q0 = 0;
      while (lane >= q0 + 6 - r) { q0 += 6 - r; ++r; }
      const int cc = r + lane - q0;
      D.H[(size_t)(o + r) * D.P + o + cc] += sum;
      if (cc != r) D.H[(size_t)(o + cc) * D.P + o + r] += sum;
    }
  }
}
// inertial + random-walk edges: one 64-thread workgroup per link; thread 0 evaluates the edge (error, 9 x 24 Jacobian) into LDS, all
// threads multiply out J^T Omega J
// One launch per colour: the links of a launch share no keyframe (a chain of consecutive keyframes has two colours), so every entry of H
// receives its contributions — the keyframe's visual block, then its links colour by colour — in the same order in every run.
__global__ __launch_bounds__(64) void k_iba_links(IbaDev D, int base) {
  __shared__ double J[216], OJ[216], Oe[9];
  __shared__ double sw;
  if (iba_no_build(D)) return;
  const int i = D.linkOrder[base + blockIdx.x], tid = threadIdx.x;
  const int k1 = D.iKF1[i], k2 = D.iKF2[i];
  for (int k = tid; k < 216; k += 64) J[k] = 0;
  __syncthreads();
  const double* er = D.iErr + 9 * (size_t)i;   // errors of computeActiveErrors (same state)
  const double* Om = D.InfoI + (size_t)i * 81;
  if (tid == 0) {
    VIState V1, V2;
    iba_load(D.g, D.S + 33 * (size_t)k1, V1);
    iba_load(D.g, D.S + 33 * (size_t)k2, V2);
    double errNow[9];
    inertial_edge(D.iPre[i], V1, V2, nullptr, true, errNow, J);
    sw = D.iRobust[i] ? huber_w(sqrt(16.92), iba_quad(er, Om, 9)) : 1.0;
  }
  __syncthreads();
  for (int k = tid; k < 216 + 9; k += 64) {
    if (k < 216) { const int r = k / 24, c = k - r * 24; double sm = 0; for (int l = 0; l < 9; ++l) sm += Om[r * 9 + l] * J[l * 24 + c]; OJ[k] = sm; }
    else { const int r = k - 216; double sm = 0; for (int l = 0; l < 9; ++l) sm += Om[r * 9 + l] * er[l]; Oe[r] = sm; }
  }
  __syncthreads();
  const double w = sw;
  const int c1 = D.off[k1], c2 = D.off[k2];   // (a link's endpoints are fixed or 15 columns wide)
  for (int idx = tid; idx < 24 * 24 + 24; idx += 64) {
    const int a = idx < 576 ? idx / 24 : idx - 576;
    const int ca = a < 15 ? (c1 >= 0 ? c1 + a : -1) : (c2 >= 0 ? c2 + (a - 15) : -1);
    if (ca < 0) continue;
    if (idx < 576) {
      const int b2 = idx - a * 24;
      const int cb = b2 < 15 ? (c1 >= 0 ? c1 + b2 : -1) : (c2 >= 0 ? c2 + (b2 - 15) : -1);
      if (cb < 0) continue;
      double h = 0;
      for (int k = 0; k < 9; ++k) h += J[k * 24 + a] * OJ[k * 24 + b2];
      if (h != 0.0) unsafeAtomicAdd(&D.H[(size_t)ca * D.P + cb], w * h);
    } else {
      double sm = 0;
      for (int k = 0; k < 9; ++k) sm += J[k * 24 + a] * Oe[k];
      unsafeAtomicAdd(&D.b[ca], -w * sm);
    }
  }
  __syncthreads();   // (the random-walk terms land on entries of the bias blocks the loop above has added to: after it, not in a race with it)
  if (tid < 18) {   // EdgeGyroRW / EdgeAccRW: e = bias2 - bias1; thread = (type, row r, column c)
    const int t = tid / 9, r = (tid % 9) / 3, c = tid % 3;
    const double* I3 = (t == 0 ? D.InfoG : D.InfoA) + (size_t)i * 9;
    const double* e3 = (t == 0 ? D.gErr : D.aErr) + 3 * (size_t)i;
    const int o1 = c1 >= 0 ? c1 + 9 + 3 * t : -1, o2 = c2 >= 0 ? c2 + 9 + 3 * t : -1;
    const double v = I3[r * 3 + c];
    if (o2 >= 0) unsafeAtomicAdd(&D.H[(size_t)(o2 + r) * D.P + o2 + c], v);
    if (o1 >= 0) unsafeAtomicAdd(&D.H[(size_t)(o1 + r) * D.P + o1 + c], v);
    if (o1 >= 0 && o2 >= 0) { unsafeAtomicAdd(&D.H[(size_t)(o1 + r) * D.P + o2 + c], -v); unsafeAtomicAdd(&D.H[(size_t)(o2 + r) * D.P + o1 + c], -v); }
    if (c == 0) {
      double sm = 0;
      for (int k = 0; k < 3; ++k) sm += I3[r * 3 + k] * e3[k];
      if (o2 >= 0) unsafeAtomicAdd(&D.b[o2 + r], -sm);
      if (o1 >= 0) unsafeAtomicAdd(&D.b[o1 + r], sm);
    }
  }
}
__device__ __forceinline__ bool inv3(const double* D3, double* I) {
  const double a = D3[0], b = D3[1], c = D3[2], d = D3[3], e = D3[4], f = D3[5], g = D3[6], h = D3[7], i = D3[8];
  const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
  const double det = a * A + b * B + c * C;
  if (det == 0.0) { for (int k = 0; k < 9; ++k) I[k] = 0; return false; }
  const double inv = 1.0 / det;
  I[0] = A * inv; I[1] = -(b * i - c * h) * inv; I[2] = (b * f - c * e) * inv;
  I[3] = B * inv; I[4] = (a * i - c * g) * inv; I[5] = -(a * f - c * d) * inv;
  I[6] = C * inv; I[7] = -(a * h - b * g) * inv; I[8] = (a * e - b * d) * inv;
  return true;
}
// MFMA operands of the Schur complement (schur_mfma.h).  W: Hpl of every observation of an optimizable keyframe and b_l in the extra
// column (once per outer iteration, after buildSystem); WD = Hpl (Hll + lambda I)^-1 (every trial).
// Hpl of (keyframe column c1, point m) as the MFMA operands need it: on a fisheye rig a keyframe may observe a point with both
// cameras, i.e. through two edges — the first of them (lowest edge index) carries the sum, the others nothing.
__device__ __forceinline__ bool iba_pair_block(const IbaDev& D, int e, int c1, int m, double* __restrict__ B) {
  for (int q = 0; q < 18; ++q) B[q] = D.Hpl[(size_t)e * 18 + q];
  for (int k = D.ptStart[m]; k < D.ptStart[m + 1]; ++k) {
    const int e2 = D.ptEdges[k];
    if (e2 == e || D.col[D.eKF[e2]] != c1) continue;
    if (e2 < e) return false;
    for (int q = 0; q < 18; ++q) B[q] += D.Hpl[(size_t)e2 * 18 + q];
  }
  return true;
}
__global__ __launch_bounds__(256) void k_iba_pack_w(IbaDev D) {
  if (iba_no_build(D)) return;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int M = 6 * D.nFree;
  if (t < D.nE) {
    const int c1 = D.col[D.eKF[t]];
    const int m = D.eMP[t];
    double B1[18];
    if (c1 >= 0 && iba_pair_block(D, t, c1, m, B1)) {
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) D.sW[(size_t)(3 * m + c) * D.sMp + 6 * c1 + r] = B1[r * 3 + c];
    }
  }
  if (t < 3 * D.nMP) D.sW[(size_t)t * D.sMp + M] = D.b[D.P + t];
}
// (the launch also sets Hs = H + lambda I, bs = b on its first P * P + P threads: one launch fewer per trial)
__global__ __launch_bounds__(256) void k_iba_pack_wd(IbaDev D) {
  if (iba_done(D)) return;
  const double lambda = D.lmd[IBA_LMD_LAMBDA];
  const int t = blockIdx.x * 256 + threadIdx.x;
  {
    const int n = D.P * D.P;
    if (t < n) { const int r = t / D.P, c = t - r * D.P; D.Hs[t] = D.H[t] + (r == c ? lambda : 0.0); }
    else if (t - n < D.P) D.bs[t - n] = D.b[t - n];
  }
  if (t >= D.nE) return;
  const int c1 = D.col[D.eKF[t]];
  if (c1 < 0) return;
  const int m = D.eMP[t];
  double B1[18];
  if (!iba_pair_block(D, t, c1, m, B1)) return;
  double Dm[9], Di[9];
  for (int k = 0; k < 9; ++k) Dm[k] = D.Hll[(size_t)m * 9 + k];
  Dm[0] += lambda; Dm[4] += lambda; Dm[8] += lambda;
  inv3(Dm, Di);
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      D.sWD[(size_t)(3 * m + c) * D.sMp + 6 * c1 + r] = B1[r * 3] * Di[c] + B1[r * 3 + 1] * Di[3 + c] + B1[r * 3 + 2] * Di[6 + c];
}
// Hs(pose rows / columns) -= C, bs(pose rows) -= C[:, M], from the partial products (four lanes per element, fixed order)
__global__ __launch_bounds__(256) void k_iba_schur_finish(IbaDev D) {
  if (iba_done(D)) return;
  const int t = blockIdx.x * 256 + threadIdx.x, gid = t >> 2, q = t & 3;
  const int M = 6 * D.nFree;
  const bool mat = gid < M * M, rhs = !mat && gid < M * M + M;
  int r = 0, c = M;
  if (mat) { r = gid / M; c = gid - r * M; } else if (rhs) r = gid - M * M;
  const int i = r < c ? r : c, j = r < c ? c : r;
  const double cs = morbschur::schur_sum4(D.sPart, D.sBlkIndex, D.sNb, D.sNblk, D.sNsplit, (mat || rhs) ? i : 0, (mat || rhs) ? j : 0, q);
  if (q != 0) return;
  if (mat) D.Hs[(size_t)(D.colOff[r / 6] + r % 6) * D.P + D.colOff[c / 6] + c % 6] -= cs;
  else if (rhs) D.bs[D.colOff[r / 6] + r % 6] -= cs;
}
// dense LDL^T + solve with the lower triangle resident in LDS (dense_ldlt.h): windows up to 15 N = 150 (n <= 163 fits)
__global__ __launch_bounds__(morbdense::LT) void k_iba_solve_lds(IbaDev D) {
  extern __shared__ double sLd[];
  __shared__ int sOk;
  if (iba_done(D)) return;
  const bool ok = morbdense::ldlt_solve<true>(D.Hs, D.bs, D.x, D.P, sLd, &sOk);
  if (threadIdx.x == 0) D.scal[2] = ok ? 1.0 : 0.0;
}
// larger windows (bLarge, or more than 10 optimizable keyframes): the matrix stays in global memory, one 16-column panel at a time in LDS
// (dense_ldlt.h: ldlt_solve_global; the panel copies move to a global scratch when even they do not fit LDS, P > 525)
__global__ __launch_bounds__(morbdense::GT) void k_iba_solve_blocked(IbaDev D, int panelInLds) {
  extern __shared__ double sm[];   // dblk[NB * NBP] | y[n] | (pnlL | pnlU when they fit)
  __shared__ int sOk;
  if (iba_done(D)) return;
  double* pnl = panelInLds ? sm + morbdense::global_lds_doubles(D.P) : D.pnlG;
  const bool ok = morbdense::ldlt_solve_global<true>(D.Hs, D.bs, D.x, D.P, pnl, sm, &sOk);
  if (threadIdx.x == 0) D.scal[2] = ok ? 1.0 : 0.0;
}

// back-substitution of the points + oplus of every vertex + the LM scale  sum x (lambda x + b) -> partScale[block]
__global__ __launch_bounds__(256) void k_iba_update(IbaDev D) {
  if (iba_done(D)) return;
  const double lambda = D.lmd[IBA_LMD_LAMBDA];
  const int t = blockIdx.x * 256 + threadIdx.x;
  double sc = 0;
  if (t < D.nMP) {
    const int l = t;
    double Dm[9], Di[9];
    for (int k = 0; k < 9; ++k) Dm[k] = D.Hll[(size_t)l * 9 + k];
    Dm[0] += lambda; Dm[4] += lambda; Dm[8] += lambda;
    inv3(Dm, Di);
    const double* bl = D.b + D.P + 3 * (size_t)l;
    double cl[3] = {bl[0], bl[1], bl[2]};
    for (int k = D.ptStart[l]; k < D.ptStart[l + 1]; ++k) {
      const int e = D.ptEdges[k];
      const int c1 = D.col[D.eKF[e]];
      if (c1 < 0) continue;
      const double* B = D.Hpl + (size_t)e * 18;
      const double* xp = D.x + D.colOff[c1];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 6; ++r) cl[c] -= B[r * 3 + c] * xp[r];
    }
    for (int r = 0; r < 3; ++r) {
      const double xl = Di[r * 3] * cl[0] + Di[r * 3 + 1] * cl[1] + Di[r * 3 + 2] * cl[2];
      D.x[D.P + 3 * (size_t)l + r] = xl;
      D.pts[3 * (size_t)l + r] += xl;
      sc += xl * (lambda * xl + bl[r]);
    }
  } else if (t - D.nMP < D.nKF) {
    const int k = t - D.nMP;
    const int o = D.off[k];
    if (o >= 0) {
      VIState V;
      iba_load(D.g, D.S + 33 * (size_t)k, V);
      const int w = D.wid[k];   // a keyframe free in the pose only owns six columns: its velocity and biases do not move
      double dx[15];
#pragma unroll
      for (int q = 0; q < 15; ++q) { dx[q] = 0.0; if (q < w) { dx[q] = D.x[o + q]; sc += dx[q] * (lambda * dx[q] + D.b[o + q]); } }
      apply_update(D.g, V, dx);
      iba_store(V, D.S + 33 * (size_t)k);
    }
  }
  const double bs = block_sum(sc);
  if (threadIdx.x == 0) D.partScale[blockIdx.x] = bs;
}
// erase flags (:2773-2801) from the errors of the last computeActiveErrors, and the float outputs
__global__ __launch_bounds__(256) void k_iba_finish(IbaDev D, uint8_t* __restrict__ erase, float* __restrict__ kfOut, float* __restrict__ mpOut) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < D.nE) {
    const float* o = D.eObs + 3 * (size_t)t;
    const bool st = !D.g.rig && !(o[2] < 0);
    const double c = iba_vis_chi2(D, t);
    bool er;
    if (st) er = c > (double)7.815f;
    else {
      const bool bClose = D.mpClose[D.eMP[t]] != 0;
      VIState V;
      iba_load(D.g, D.S + 33 * (size_t)D.eKF[t], V);
      const int cam = D.eRight && D.eRight[t] ? 1 : 0;
      const double r6 = cam ? V.Rcw1[6] : V.Rcw[6], r7 = cam ? V.Rcw1[7] : V.Rcw[7], r8 = cam ? V.Rcw1[8] : V.Rcw[8], tz = cam ? V.tcw1[2] : V.tcw[2];
      const double* X = D.pts + 3 * (size_t)D.eMP[t];
      const bool depthPos = (r6 * X[0] + r7 * X[1] + r8 * X[2] + tz) > 0.0;
      er = (c > (double)5.991f && !bClose) || (c > (double)(1.5f * 5.991f) && bClose) || !depthPos;
      if (D.eraseChi2Only) er = c > (double)5.991f;   // MergeInertialBA (:4287-4310): no depth test, no mTrackDepth rule
    }
    erase[t] = er ? 1 : 0;
  }
  if (t < D.nKF && D.off[t] >= 0) {   // (pose-only keyframes: Rwb, twb; their velocity and bias floats stay the caller's)
    const int n = D.wid[t] == 15 ? 21 : 12;
    for (int k = 0; k < n; ++k) kfOut[21 * (size_t)t + k] = (float)D.S[33 * (size_t)t + k];
  }
  if (t < 3 * D.nMP) mpOut[t] = (float)D.pts[t];
}

}  // namespace

extern "C" {

static int iba_fail(const char* what) { set_error("%s", what); return MORB_ERR_HIP; }

// What LocalInertialBA uploads besides the caller's arrays: CSR lists (ba_host.h), 64-edge chunks of the optimizable keyframes'
// edges, the inertial links by colour, and the Schur product's block lists.
struct IbaLayout {
  std::vector<int> col, ptStart, ptEdges, kfStart, kfEdges, chunkKF, chunkStart, chunkEnd, linkOrder, colourStart, blkIndex;
  std::vector<int2> blocks;
  std::vector<int> off, wid, colOff;   // the reduced system's columns: per keyframe (first column or -1, width), per pose block
  int nFree = 0, P = 0;
  morbschur::Plan splan;
};

// The plan of an optimiser on this graph, as data: LocalInertialBA (:2324-2897) and MergeInertialBA (:3853-4389) run the same kernels.
struct IbaPlan {
  int iterations; double lambda0;   // optimize(n), setUserLambdaInit
  bool eraseChi2Only;               // erase by chi2 alone | LocalInertialBA's rule with the depth test and mTrackDepth
  bool failTest;                    // "FAIL LOCAL-INERTIAL BA": nothing is written back when the error doubled
  bool poseOnlyKinds;               // kfKind 3 (free in the pose only) is accepted
  const char* who;
};

static int iba_layout(int nKF, const uint8_t* kfKind, int nMP, int nE, const int* eKF, const int* eMP, int nI, const int* iKF1, const int* iKF2,
                      bool poseOnlyKinds, IbaLayout& L) {
  L.col.assign(nKF, -1); L.off.assign(nKF, -1); L.wid.assign(nKF, 0);
  for (int k = 0; k < nKF; ++k) {
    const int w = kfKind[k] == 0 ? 15 : (poseOnlyKinds && kfKind[k] == 3) ? 6 : 0;   // (pose-only keyframes are not padded to 15 columns)
    if (!w) continue;
    L.col[k] = L.nFree++; L.off[k] = L.P; L.wid[k] = w; L.colOff.push_back(L.P); L.P += w;
  }
  MORB_REQUIRE(L.nFree > 0, MORB_ERR_INVALID, "no optimizable keyframe");
  for (int e = 0; e < nE; ++e) MORB_REQUIRE(eKF[e] >= 0 && eKF[e] < nKF && eMP[e] >= 0 && eMP[e] < nMP, MORB_ERR_INVALID, "edge index out of range");
  for (int i = 0; i < nI; ++i) MORB_REQUIRE(iKF1[i] >= 0 && iKF1[i] < nKF && iKF2[i] >= 0 && iKF2[i] < nKF, MORB_ERR_INVALID, "link index out of range");
  if (poseOnlyKinds)   // a link's endpoints carry velocity and biases: free with 15 unknowns, or fixed with an IMU state
    for (int i = 0; i < nI; ++i) MORB_REQUIRE(kfKind[iKF1[i]] <= 1 && kfKind[iKF2[i]] <= 1, MORB_ERR_INVALID, "link ends on a keyframe without velocity and biases");
  csr_by_key(eMP, nE, nMP, L.ptStart, L.ptEdges);
  csr_by_key(eKF, nE, nKF, L.kfStart, L.kfEdges, L.col.data());   // (compact: the optimizable keyframes' edges only)
  chunks_of(L.kfStart, L.col.data(), 64, L.chunkKF, L.chunkStart, L.chunkEnd);
  // colour the inertial links so that links of one colour share no keyframe (greedy; a chain of consecutive keyframes alternates 0 / 1)
  std::vector<int> colour(nI, 0);
  int nColours = 0;
  for (int i = 0; i < nI; ++i) {
    int c = 0;
    for (bool clash = true; clash; ) {
      clash = false;
      for (int j = 0; j < i && !clash; ++j)
        clash = colour[j] == c && (iKF1[j] == iKF1[i] || iKF1[j] == iKF2[i] || iKF2[j] == iKF1[i] || iKF2[j] == iKF2[i]);
      if (clash) ++c;
    }
    colour[i] = c; nColours = std::max(nColours, c + 1);
  }
  for (int c = 0; c < nColours; ++c) { L.colourStart.push_back((int)L.linkOrder.size()); for (int i = 0; i < nI; ++i) if (colour[i] == c) L.linkOrder.push_back(i); }
  L.colourStart.push_back((int)L.linkOrder.size());
  L.splan = morbschur::make_plan(6 * L.nFree + 1, 3 * nMP);
  schur_block_lists(L.splan.nb, L.blocks, L.blkIndex);
  return MORB_OK;
}

// Levenberg-Marquardt with the control flow on the device (as grid-mode LocalBA, local_ba.hip): one slot = one trial; the host queues
// slots one ahead of the decisions and stops when the mapped `done` word appears (ba_host.h); kernels queued behind the last decision return at once.
// Leaves the loop's counters in *outer / *trials and the chi2 of the last evaluated trial in *lastChi.
// stopFlag: the caller's *pbStopFlag or NULL; the queue's tick forwards it to a spare mapped word ([2]) the decision kernels poll.
static int iba_lm_loop(morb_optimizer* o, hipStream_t st, IbaDev& D, const IbaLayout& L, double chi, const IbaPlan& plan, const volatile uint8_t* stopFlag,
                       size_t denseLds, size_t blockedLds, int panelInLds, int* outer, int* trials, double* lastChi) {
  const int nKF = D.nKF, nMP = D.nMP, nE = D.nE, nI = D.nI, P = D.P, nChunks = D.nChunks, Mpose = 6 * L.nFree;
  const size_t nS = (size_t)D.nS, nPts = (size_t)D.nPts;
  int *hostw = nullptr, *hostwDev = nullptr;
  MORB_REQUIRE(morb_optimizer_lm_words(o, &hostw, &hostwDev) == MORB_OK, MORB_ERR_HIP, "cannot map the LM state words");
  D.lmHost = hostwDev;
  D.optIt = plan.iterations; D.eraseChi2Only = plan.eraseChi2Only ? 1 : 0;
  D.stopWord = stopFlag ? hostwDev + 2 : nullptr;
  auto forwardStop = [&]() { if (stopFlag && *stopFlag) __atomic_store_n(hostw + 2, 1, __ATOMIC_RELEASE); };
  reset_lm_words(hostw, 2, hostw + 2);
  forwardStop();
  hipLaunchKernelGGL(k_iba_lm_init, dim3(1), dim3(1), 0, st, D, chi, plan.lambda0);
  const int beginGrid = div_up((int)std::max<size_t>(std::max<size_t>(std::max<size_t>(nS, nPts), (size_t)nMP * 8 /* k_iba_points: eight lanes per point */), std::max<size_t>((size_t)P * P, (size_t)18 * nE)), 256);
  const int q = lm_slot_queue(120, hostw + 0, hostw + 1, [&](int) {
    // backup / restore, then buildSystem (which runs only when the previous trial was accepted)
    hipLaunchKernelGGL(k_iba_points, dim3(beginGrid), dim3(256), 0, st, D);
    if (nChunks) hipLaunchKernelGGL(k_iba_kf, dim3(div_up(nChunks, 4)), dim3(256), 0, st, D);
    for (size_t c = 0; c + 1 < L.colourStart.size(); ++c)
      hipLaunchKernelGGL(k_iba_links, dim3(L.colourStart[c + 1] - L.colourStart[c]), dim3(64), 0, st, D, L.colourStart[c]);
    hipLaunchKernelGGL(k_iba_pack_w, dim3(div_up(std::max(nE, 3 * nMP), 256)), dim3(256), 0, st, D);
    // the trial: Schur complement of the points on the FP64 matrix cores, one dense product for matrix and right-hand side
    hipLaunchKernelGGL(k_iba_pack_wd, dim3(div_up(std::max(nE, P * P + P), 256)), dim3(256), 0, st, D);
    hipLaunchKernelGGL(morbschur::k_schur_mfma, dim3(L.splan.nblk, L.splan.nsplit), dim3(64), 0, st, (const double*)D.sWD, (const double*)D.sW,
                       L.splan.Mp, L.splan.ksteps, L.splan.stepsPerSplit, D.sBlocks, D.sPart, (const int*)(D.lmi + IBA_LM_DONE));
    hipLaunchKernelGGL(k_iba_schur_finish, dim3(div_up(4 * (Mpose * Mpose + Mpose), 256)), dim3(256), 0, st, D);
    if (denseLds) hipLaunchKernelGGL(k_iba_solve_lds, dim3(1), dim3(morbdense::LT), denseLds, st, D);
    else hipLaunchKernelGGL(k_iba_solve_blocked, dim3(1), dim3(morbdense::GT), blockedLds, st, D, panelInLds);
    // a failed solve leaves x as it was (zero at the first trial): g2o still applies the update
    hipLaunchKernelGGL(k_iba_update, dim3(div_up(nMP + nKF, 256)), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_iba_errors, dim3(div_up(nE + nI, 256)), dim3(256), 0, st, D, 1);
    if (hipGetLastError() != hipSuccess) { set_error("%s trial failed", plan.who); return (int)MORB_ERR_HIP; }
    return (int)MORB_OK;
  }, [&]() { return stream_look(st, plan.who); }, forwardStop);   // (LocalInertialBA's caller has no flag to forward)
  if (q < 0) return MORB_ERR_HIP;
  // (a queue that ran out of slots without `done` is drained by the read-back below, before the words are reset again)
  hipLaunchKernelGGL(k_iba_end, dim3(div_up((int)std::max<size_t>(nS, nPts), 256)), dim3(256), 0, st, D);
  int hi[16]; double hd[8];
  if (hipMemcpyAsync(hi, D.lmi, sizeof hi, hipMemcpyDeviceToHost, st) != hipSuccess || hipMemcpyAsync(hd, D.lmd, sizeof hd, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess)
  { set_error("%s failed", plan.who); return MORB_ERR_HIP; }
  *outer = hi[IBA_LM_ITS]; *trials = hi[IBA_LM_TRIALS]; *lastChi = hd[IBA_LMD_LASTCHI];
  return MORB_OK;
}

// static void Optimizer::LocalInertialBA(KeyFrame*, bool* pbStopFlag, Map*, int&, int&, int&, int&, bool bLarge, bool bRecInit) and
// static void Optimizer::MergeInertialBA(KeyFrame*, KeyFrame*, bool* pbStopFlag, Map*, LoopClosing::KeyFrameAndPose&) on the flattened
// graph (see include/morb_hip.h), told apart by the plan.  HOST pointers.  eRight / rig28 != NULL: fisheye rig.  stopFlag: the caller's
// *pbStopFlag or NULL; set at entry, nothing runs and nothing is written (stats3[2] = 0).
static int iba_impl(morb_optimizer* o, const IbaPlan& plan, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos,
                    const uint8_t* mpClose, int nE, const int* eKF, const int* eMP, const float* eObs, const float* eInvSigma2,
                    int nI, const int* iKF1, const int* iKF2, const morb_imu_preintegrated* iPre, const uint8_t* iRobust,
                    const float* iInfoScale, float fx, float fy, float cx, float cy, float bf, const float* Tbc12,
                    const volatile uint8_t* stopFlag, uint8_t* eraseFlag, int* stats3, const uint8_t* eRight, const float* rig28) {
  MORB_REQUIRE((eRight == nullptr) == (rig28 == nullptr), MORB_ERR_INVALID, "eRight and rig28 go together");
  MORB_REQUIRE(o && kfState21 && kfKind && mpPos && mpClose && eKF && eMP && eObs && eInvSigma2 && iKF1 && iKF2 && iPre && iRobust &&
                   iInfoScale && Tbc12 && eraseFlag, MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nKF > 0 && nMP > 0 && nE > 0 && nI >= 0, MORB_ERR_INVALID, "bad sizes");
  MORB_ENTER(st, o, nullptr);
  // ---- host-side graph layout
  IbaLayout L;
  { const int rc = iba_layout(nKF, kfKind, nMP, nE, eKF, eMP, nI, iKF1, iKF2, plan.poseOnlyKinds, L); if (rc != MORB_OK) return rc; }
  const int P = L.P, nChunks = (int)L.chunkKF.size();
  if (stopFlag && *stopFlag) { if (stats3) { stats3[0] = 0; stats3[1] = 0; stats3[2] = 0; } return MORB_OK; }   // `if (*pbStopFlag) return;` (:4276)

  // ---- device memory: every array is carved from the handle's grow-only workspace (ba_host.h): host -> device arrays first, each
  // copied into a pinned mirror of that region which crosses PCIe in ONE copy (twenty pageable hipMemcpyAsync calls, each staged and
  // synchronised by the runtime, were ~0.25 ms of a 1.8 ms call), the device-only arrays behind them
  const size_t nS = (size_t)33 * nKF, nPts = (size_t)3 * nMP, nX = (size_t)P + 3 * nMP, nI1 = (size_t)std::max(nI, 1);
  IbaDev D;
  memset(&D, 0, sizeof D);
  D.nKF = nKF; D.nMP = nMP; D.nE = nE; D.nI = nI; D.P = P; D.nChunks = nChunks; D.nFree = L.nFree;
  D.nS = (int)nS; D.nPts = (int)nPts; D.nbUpdate = div_up(nMP + nKF, 256);
  D.sMp = L.splan.Mp; D.sNb = L.splan.nb; D.sNblk = L.splan.nblk; D.sNsplit = L.splan.nsplit;
  make_geom(Tbc12, fx, fy, cx, cy, bf, rig28, D.g);
  float *d_scale = nullptr, *d_kfIn = nullptr, *d_mpIn = nullptr; uint8_t* d_erase = nullptr;
  ArenaCarver A;
  auto carve = [&]() {
    D.eKF = (const int*)A.take(eKF, sizeof(int) * nE); D.eMP = (const int*)A.take(eMP, sizeof(int) * nE);
    D.eObs = (const float*)A.take(eObs, sizeof(float) * 3 * nE); D.eInfo = (const float*)A.take(eInvSigma2, sizeof(float) * nE);
    D.ptStart = (const int*)A.take(L.ptStart.data(), sizeof(int) * (nMP + 1)); D.ptEdges = (const int*)A.take(L.ptEdges.data(), sizeof(int) * nE);
    D.kfEdges = (const int*)A.take(L.kfEdges.data(), sizeof(int) * L.kfEdges.size());
    D.chunkKF = (const int*)A.take(L.chunkKF.data(), sizeof(int) * nChunks); D.chunkStart = (const int*)A.take(L.chunkStart.data(), sizeof(int) * nChunks);
    D.chunkEnd = (const int*)A.take(L.chunkEnd.data(), sizeof(int) * nChunks); D.col = (const int*)A.take(L.col.data(), sizeof(int) * nKF);
    D.off = (const int*)A.take(L.off.data(), sizeof(int) * nKF); D.wid = (const int*)A.take(L.wid.data(), sizeof(int) * nKF);
    D.colOff = (const int*)A.take(L.colOff.data(), sizeof(int) * L.nFree);
    D.iKF1 = (const int*)A.take(iKF1, sizeof(int) * nI); D.iKF2 = (const int*)A.take(iKF2, sizeof(int) * nI);
    D.iPre = (const morb_imu_preintegrated*)A.take(iPre, sizeof(morb_imu_preintegrated) * nI);
    D.iRobust = (const uint8_t*)A.take(iRobust, nI); D.mpClose = (const uint8_t*)A.take(mpClose, nMP);
    d_scale = (float*)A.take(iInfoScale, sizeof(float) * nI); d_kfIn = (float*)A.take(kfState21, sizeof(float) * 21 * nKF);
    d_mpIn = (float*)A.take(mpPos, sizeof(float) * 3 * nMP);
    D.eRight = eRight ? (const uint8_t*)A.take(eRight, nE) : nullptr;
    D.sBlocks = (const int2*)A.take(L.blocks.data(), sizeof(int2) * L.blocks.size()); D.sBlkIndex = (const int*)A.take(L.blkIndex.data(), sizeof(int) * L.blkIndex.size());
    D.linkOrder = (const int*)A.take(L.linkOrder.data(), sizeof(int) * nI);
    D.kfPart = (double*)A.take(nullptr, sizeof(double) * 27 * (size_t)nChunks); D.kfTicket = (int*)A.take(nullptr, sizeof(int) * (size_t)nKF);
    D.S = (double*)A.take(nullptr, sizeof(double) * nS); D.Sbk = (double*)A.take(nullptr, sizeof(double) * nS);
    D.pts = (double*)A.take(nullptr, sizeof(double) * nPts); D.ptsBk = (double*)A.take(nullptr, sizeof(double) * nPts);
    D.lmd = (double*)A.take(nullptr, sizeof(double) * 8); D.lmi = (int*)A.take(nullptr, sizeof(int) * 16);
    D.vErr = (double*)A.take(nullptr, sizeof(double) * 3 * nE); D.iErr = (double*)A.take(nullptr, sizeof(double) * 9 * nI1);
    D.gErr = (double*)A.take(nullptr, sizeof(double) * 3 * nI1); D.aErr = (double*)A.take(nullptr, sizeof(double) * 3 * nI1);
    D.InfoI = (double*)A.take(nullptr, sizeof(double) * 81 * nI1); D.InfoG = (double*)A.take(nullptr, sizeof(double) * 9 * nI1);
    D.InfoA = (double*)A.take(nullptr, sizeof(double) * 9 * nI1); D.H = (double*)A.take(nullptr, sizeof(double) * (size_t)P * P); D.Hs = (double*)A.take(nullptr, sizeof(double) * (size_t)P * P);
    D.b = (double*)A.take(nullptr, sizeof(double) * nX); D.bs = (double*)A.take(nullptr, sizeof(double) * P); D.x = (double*)A.take(nullptr, sizeof(double) * nX);
    D.Hll = (double*)A.take(nullptr, sizeof(double) * 9 * nMP); D.Hpl = (double*)A.take(nullptr, sizeof(double) * 18 * nE); D.scal = (double*)A.take(nullptr, sizeof(double) * 4);
    D.partChi = (double*)A.take(nullptr, sizeof(double) * div_up(nE + nI, 256)); D.partScale = (double*)A.take(nullptr, sizeof(double) * D.nbUpdate);
    D.pnlG = (double*)A.take(nullptr, sizeof(double) * morbdense::global_panel_doubles(P)); d_erase = (uint8_t*)A.take(nullptr, nE);
    D.sW = (double*)A.take(nullptr, sizeof(double) * L.splan.wElems()); D.sWD = (double*)A.take(nullptr, sizeof(double) * L.splan.wElems());
    D.sPart = (double*)A.take(nullptr, sizeof(double) * L.splan.partElems());
  };
  carve();   // (dry: sizes)
  char *arena = nullptr, *stage = nullptr;
  { const int rc = grow(o->work, A.uploadBytes() + A.deviceBytes(), &arena); if (rc != MORB_OK) return rc; }
  { const int rc = grow(o->stage, A.uploadBytes(), &stage); if (rc != MORB_OK) return rc; }
  A.bind(arena, stage);
  carve();
  if (!A.ok()) { set_error("the two carve passes of %s differ", plan.who); return MORB_ERR_HIP; }
  if (hipMemcpyAsync(arena, stage, A.uploadBytes(), hipMemcpyHostToDevice, st) != hipSuccess) return MORB_ERR_HIP;   // the one upload
  // the workspace is reused from call to call: what the first kernels expect to find zero is cleared behind the carve
  (void)hipMemsetAsync(D.kfTicket, 0, sizeof(int) * (size_t)nKF, st);   // (the last chunk of a keyframe to arrive resets its counter)
  (void)hipMemsetAsync(D.lmi, 0, sizeof(int) * 16, st);   // (k_iba_errors' arrival counter is live before k_iba_lm_init)
  (void)hipMemsetAsync(D.x, 0, sizeof(double) * nX, st);   // the solver's x before the first solve
  (void)hipMemsetAsync(D.sW, 0, sizeof(double) * L.splan.wElems(), st); (void)hipMemsetAsync(D.sWD, 0, sizeof(double) * L.splan.wElems(), st);   // the operands' zero pattern is this graph's

  hipLaunchKernelGGL(k_iba_setup_kf, dim3(div_up(nKF, 64)), dim3(64), 0, st, D, d_kfIn);
  if (nI) hipLaunchKernelGGL(k_iba_setup_links, dim3(nI), dim3(64), 0, st, D, d_scale);
  hipLaunchKernelGGL(k_iba_setup_pts, dim3(div_up((int)nPts, 256)), dim3(256), 0, st, D, (const float*)d_mpIn);   // points to FP64
  size_t blockedLds = sizeof(double) * (morbdense::global_lds_doubles(P) + morbdense::global_panel_doubles(P));
  const int panelInLds = blockedLds <= morbdense::GLOBAL_SOLVER_LIMIT ? 1 : 0;
  if (!panelInLds) blockedLds = sizeof(double) * morbdense::global_lds_doubles(P);
  MORB_REQUIRE(blockedLds <= morbdense::GLOBAL_SOLVER_LIMIT, MORB_ERR_CAPACITY, "window too large for the dense solver");
  if (blockedLds > 48 * 1024)
    MORB_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_iba_solve_blocked), hipFuncAttributeMaxDynamicSharedMemorySize, (int)blockedLds));
  size_t denseLds = sizeof(double) * morbdense::lds_doubles(P);
  if (denseLds > morbdense::LDS_SOLVER_LIMIT) denseLds = 0;   // larger windows (bLarge) use the global-memory solver
  if (denseLds) MORB_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_iba_solve_lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)morbdense::LDS_SOLVER_LIMIT));
  double h[4];   // computeActiveErrors + activeRobustChi2
  if (hipMemsetAsync(D.scal, 0, sizeof(double) * 4, st) != hipSuccess) return iba_fail("k_iba_errors failed");
  hipLaunchKernelGGL(k_iba_errors, dim3(div_up(nE + nI, 256)), dim3(256), 0, st, D, 0);
  if (hipMemcpyAsync(h, D.scal, sizeof(double) * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return iba_fail("k_iba_errors failed");
  const double chi = h[0];
  const float err0 = (float)chi;
  int trials = 0, outer = 0;
  { const int rc = iba_lm_loop(o, st, D, L, chi, plan, stopFlag, denseLds, blockedLds, panelInLds, &outer, &trials, &h[0]); if (rc != MORB_OK) return rc; }
  // ---- read-back.  activeRobustChi2 of the last computed errors = h[0] of the last trial (or the initial one)
  const float errEnd = (float)(trials ? h[0] : chi);
  int okFlag = 1;
  if ((2 * err0 < errEnd || std::isnan(err0) || std::isnan(errEnd)) && plan.failTest) okFlag = 0;   // "FAIL LOCAL-INERTIAL BA" (:2808-2813)
  memset(eraseFlag, 0, nE);
  if (okFlag) {
    hipLaunchKernelGGL(k_iba_finish, dim3(div_up(std::max(nE, std::max(nKF, 3 * nMP)), 256)), dim3(256), 0, st, D, d_erase, d_kfIn, d_mpIn);
    (void)hipMemcpyAsync(eraseFlag, d_erase, nE, hipMemcpyDeviceToHost, st);
    (void)hipMemcpyAsync(kfState21, d_kfIn, sizeof(float) * 21 * nKF, hipMemcpyDeviceToHost, st);
    (void)hipMemcpyAsync(mpPos, d_mpIn, sizeof(float) * 3 * nMP, hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) != hipSuccess) { set_error("%s read-back failed", plan.who); return MORB_ERR_HIP; }
  }
  if (stats3) { stats3[0] = outer; stats3[1] = trials; stats3[2] = okFlag; }
  return MORB_OK;
}

// :2324-2897: optimize(10) from lambda 1 (bLarge: optimize(4) from 1e-2, and no FAIL test)
static IbaPlan local_inertial_plan(int bLarge) { return IbaPlan{bLarge ? 4 : 10, bLarge ? 1e-2 : 1e0, false, !bLarge, false, "LocalInertialBA"}; }

int morb_local_inertial_ba(morb_optimizer* o, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos,
                           const uint8_t* mpClose, int nE, const int* eKF, const int* eMP, const float* eObs, const float* eInvSigma2,
                           int nI, const int* iKF1, const int* iKF2, const morb_imu_preintegrated* iPre, const uint8_t* iRobust,
                           const float* iInfoScale, float fx, float fy, float cx, float cy, float bf, const float* Tbc12, int bLarge,
                           uint8_t* eraseFlag, int* stats3) {
  return iba_impl(o, local_inertial_plan(bLarge), nKF, kfState21, kfKind, nMP, mpPos, mpClose, nE, eKF, eMP, eObs, eInvSigma2, nI, iKF1, iKF2, iPre,
                  iRobust, iInfoScale, fx, fy, cx, cy, bf, Tbc12, nullptr, eraseFlag, stats3, nullptr, nullptr);
}
int morb_local_inertial_ba_fisheye(morb_optimizer* o, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos,
                                   const uint8_t* mpClose, int nE, const int* eKF, const int* eMP, const float* eObs, const uint8_t* eRight,
                                   const float* eInvSigma2, int nI, const int* iKF1, const int* iKF2, const morb_imu_preintegrated* iPre,
                                   const uint8_t* iRobust, const float* iInfoScale, const float* rig28, const float* Tbc12, int bLarge,
                                   uint8_t* eraseFlag, int* stats3) {
  MORB_REQUIRE(eRight && rig28, MORB_ERR_INVALID, "NULL argument");
  return iba_impl(o, local_inertial_plan(bLarge), nKF, kfState21, kfKind, nMP, mpPos, mpClose, nE, eKF, eMP, eObs, eInvSigma2, nI, iKF1, iKF2, iPre,
                  iRobust, iInfoScale, 0, 0, 0, 0, 0, Tbc12, nullptr, eraseFlag, stats3, eRight, rig28);
}


// :3853-4389: setUserLambdaInit(1e3), optimize(8), Huber on every inertial edge with the information as it stands, erase by chi2 alone,
// no FAIL test.  mpClose plays no part (zeros); rig28: every edge on the left KannalaBrandt8 camera (the function creates EdgeMono(0) only).
static int merge_inertial_ba_impl(morb_optimizer* o, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos, int nE, const int* eKF,
                                  const int* eMP, const float* eObs, const float* eInvSigma2, int nI, const int* iKF1, const int* iKF2,
                                  const morb_imu_preintegrated* iPre, float fx, float fy, float cx, float cy, float bf, const float* rig28,
                                  const float* Tbc12, const uint8_t* pbStopFlag, uint8_t* eraseFlag, int* stats3) {
  MORB_REQUIRE(o && kfState21 && kfKind && mpPos && eKF && eMP && eObs && eInvSigma2 && iKF1 && iKF2 && iPre && Tbc12 && eraseFlag && stats3,
               MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nKF > 0 && nMP > 0 && nE > 0 && nI >= 0, MORB_ERR_INVALID, "bad sizes");
  for (int k = 0; k < nKF; ++k) MORB_REQUIRE(kfKind[k] <= 3, MORB_ERR_INVALID, "kfKind out of range");
  const IbaPlan plan{8, 1e3, true, false, true, "MergeInertialBA"};
  const std::vector<uint8_t> zeros((size_t)std::max(nMP, nE), 0), robust((size_t)std::max(nI, 1), 1);
  const std::vector<float> scale((size_t)std::max(nI, 1), 1.0f);
  return iba_impl(o, plan, nKF, kfState21, kfKind, nMP, mpPos, zeros.data(), nE, eKF, eMP, eObs, eInvSigma2, nI, iKF1, iKF2, iPre, robust.data(),
                  scale.data(), fx, fy, cx, cy, bf, Tbc12, pbStopFlag, eraseFlag, stats3, rig28 ? zeros.data() : nullptr, rig28);
}
int morb_merge_inertial_ba(morb_optimizer* o, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos, int nE, const int* eKF,
                           const int* eMP, const float* eObs, const float* eInvSigma2, int nI, const int* iKF1, const int* iKF2,
                           const morb_imu_preintegrated* iPre, float fx, float fy, float cx, float cy, float bf, const float* Tbc12,
                           const uint8_t* pbStopFlag, uint8_t* eraseFlag, int* stats3) {
  return merge_inertial_ba_impl(o, nKF, kfState21, kfKind, nMP, mpPos, nE, eKF, eMP, eObs, eInvSigma2, nI, iKF1, iKF2, iPre, fx, fy, cx, cy, bf,
                                nullptr, Tbc12, pbStopFlag, eraseFlag, stats3);
}
int morb_merge_inertial_ba_fisheye(morb_optimizer* o, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos, int nE,
                                   const int* eKF, const int* eMP, const float* eObs, const float* eInvSigma2, int nI, const int* iKF1,
                                   const int* iKF2, const morb_imu_preintegrated* iPre, const float* rig28, const float* Tbc12,
                                   const uint8_t* pbStopFlag, uint8_t* eraseFlag, int* stats3) {
  MORB_REQUIRE(rig28, MORB_ERR_INVALID, "NULL argument");
  return merge_inertial_ba_impl(o, nKF, kfState21, kfKind, nMP, mpPos, nE, eKF, eMP, eObs, eInvSigma2, nI, iKF1, iKF2, iPre, 0, 0, 0, 0, 0, rig28,
                                Tbc12, pbStopFlag, eraseFlag, stats3);
}

}  // extern "C"
