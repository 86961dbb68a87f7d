// Optimizer::FullInertialBA (reference src/Optimizer.cc:364-760) for MI355X (gfx950): the inertial whole-map bundle adjustment — what
// LoopClosing::RunGlobalBundleAdjustment starts behind a loop closure once the map's IMU is initialised (LoopClosing.cc:2305) and what
// LocalMapping::InitializeIMU runs behind InertialOptimization (LocalMapping.cc:1244-1249).  Every keyframe of the map with its 15-dof
// state (inertial_device.h: ImuCamPose, EdgeMono / EdgeStereo, EdgeInertial), every point behind a Schur complement, one temporal chain of
// EdgeInertial + EdgeGyroRW + EdgeAccRW — or, with bInit, ONE gyro and one accelerometer bias for the whole map, with a prior each.  It is
// LocalInertialBA's graph (inertial_ba.hip) at global_ba.hip's size: the reduced system is neither dense nor of one block width.
//   * The reduced system lives on 3 x 3 blocks: a keyframe owns 5 block rows (pose 2, velocity, gyro bias, accelerometer bias), 3 with
//     bInit, 2 when it is free in the pose only; the shared biases own the last 2, whose envelope covers every linked keyframe: one long
//     row, like a loop edge's in the pose graphs.  Every block row of a keyframe begins at the first block row of the lowest keyframe it
//     shares a point or a link with.
//   * k_fiba_linearize: error, Huber weight and both Jacobians of every visual edge, a lane per edge.  k_fiba_links: a wave per link, lane
//     0 evaluates EdgeInertial into LDS, all lanes multiply J^T Omega J out into the link's 30 x 30 record (pose 1, v1, bg1, ba1, pose 2, v2,
//     bg2, ba2: the random-walk edges are in it).
//   * k_fiba_assemble: Hpp, bp per keyframe, Hll, bl per point, Hpl per (point, keyframe) pair, summed in edge order.
//   * k_fiba_dinv, k_fiba_schur, k_fiba_finish: global_ba.hip's sparse Schur complement — only the 6 pose columns of a keyframe meet a
//     point — cut into chunks of FIBA_CHUNK per 3 x 3 envelope block; finish adds, per envelope entry, the keyframe's visual block, its
//     links' records in link order and the priors, and takes the chunks' sums off in order.  No floating-point atomics anywhere.
//   * k_fiba_factor: H + lambda I = L D L^T over the envelope by envelope_ldlt.h, which describes the schedule: FIBA_ROWS covering rows a
//     pass, FIBA_STAGE blocks staged at a time.  A zero or NaN pivot: zero step, rejected trial.
//   * k_fiba_backsub: back-substitution (envelope_ldlt.h) and oplus (ImuCamPose::Update, additive velocity and biases; the shared biases
//     once).
//   * k_fiba_points, k_fiba_errors, k_fiba_decide: as global_ba.hip's; lambda starts at the user value 1e-5 (:384).
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
#include "inertial_device.h"

namespace {

using namespace morb;

constexpr int FIBA_NT = 256;                  // lanes of a workgroup
constexpr int FIBA_ROWS = FIBA_NT / 3;        // covering rows of 3 lines one pass of envelope_factor takes (the diagonal block's among them): 85
constexpr int FIBA_STAGE = 128;               // blocks of the column's own row envelope_factor stages in LDS at a time (9 KiB)
constexpr int FIBA_CHUNK = 64;                // Schur contributions one lane adds before the chunks are added
// envelope blocks a handle may grow to: the bytes global_ba.hip allows its 6 x 6 envelope, in 3 x 3 blocks
constexpr size_t FIBA_MAX_BLOCKS = ((size_t)1 << 22) * 49 / 9;
constexpr int FIBA_EDGE = 31;                 // doubles of a visual edge's record: Jp 3 x 6, Jl 3 x 3, -(w info) e, w info
enum { FE_JP = 0, FE_JL = 18, FE_RW = 27, FE_WO = 30 };
constexpr int FIBA_LCOLS = 30;                // columns of a link's record: pose 1 (6), v1, bg1, ba1, pose 2 (6), v2, bg2, ba2
constexpr int FIBA_LREC = FIBA_LCOLS * FIBA_LCOLS + FIBA_LCOLS;   // w J^T Omega J (+ the random-walk edges), then -w J^T Omega e

struct FibaDev {
  int nKF, nMP, nE, nI, nSys, n, P, nBlocks, nPairs, nChunks, maxIts, bInit, nChi, rbB;
  const int *eKF, *eMP;                 // [nE]
  const float *eObs, *eInfo;            // [nE][3] (x, y, uRight), [nE]
  const uint8_t* eRight;                // rig: the edge is on the right camera (NULL: pinhole)
  const int *off, *wid;                 // [nKF] first scalar row of the keyframe in the system (-1: not in it), its width 15 | 9 | 6
  const int* sysIdx;                    // [nKF] index among the keyframes of the system, or -1
  const int *kfStart, *kfEdges;         // edges by keyframe of the system, in edge order
  const int *mpStart, *mpEdges;         // edges by point, in edge order
  const int *pairStart, *pairEdges;     // [nPairs + 1] edges of a (point, keyframe of the system) pair, in edge order
  const int *pairOff, *pairMp;          // [nPairs] the keyframe's first scalar row, the point
  const int* mpPairStart;               // [nMP + 1]
  const int *kfPairStart, *kfPairs;     // [nSys + 1] pairs of a keyframe, in point order
  const int *rowFirst, *rowOff, *colStart, *colRows;   // envelope_plan.h, on 3 x 3 block rows
  const int* blkDiag;                   // [nBlocks] the block row of a diagonal block, else -1
  const int* blkVis;                    // [nBlocks] keyframe of the system * 4 + (0: pose block (0,0), 1: (1,0), 2: (1,1)), else -1
  const int* rowVis;                    // [n] keyframe of the system * 2 + pose block row, else -1
  const int *blkLinkStart, *blkLinks;   // [nBlocks + 1] link * 256 + record block row * 16 + record block column, in link order
  const int *rowLinkStart, *rowLinks;   // [n + 1] link * 16 + record block row
  const int *chunkStart, *chunkEnd;     // [nChunks] positions in ct
  const int* blkChunkStart;             // [nBlocks + 1]
  const int2* ct;                       // Schur contributions (pair * 2 + pose block row, pair * 2 + pose block column), by envelope block, in point order
  const int *iKF1, *iKF2;
  const morb_imu_preintegrated* iPre;
  const double *InfoI, *InfoG, *InfoA;  // [nI][81], [nI][9], [nI][9]
  const float *kfIn, *mpIn, *biasIn;    // the caller's floats
  double *S, *ST;                       // [nKF][33] current and trial: Rwb twb v bg ba | Rcw tcw
  double *sb, *sbT;                     // [6] the shared biases (bInit): gyro, accelerometer
  double *pt, *ptT;                     // [nMP][3]
  double* E;                            // [nE][FIBA_EDGE]
  double* LR;                           // [nI][FIBA_LREC]
  double *Hpp, *bp;                     // [nSys][36], [nSys][6]
  double *Hll, *bl, *Dinv, *xl;         // [nMP][9], [nMP][3], [nMP][9], [nMP][3]
  double *Hpl, *HplD, *hg;              // [nPairs][18] row-major 6 x 3; Hpl Dinv; [nPairs][6] Hpl (Dinv bl)
  double* part;                         // [nChunks][9]
  double *H, *L;                        // [nBlocks][9] the reduced system in the envelope; its factor
  double *b0, *b, *y, *x, *d;           // [P] the right-hand side before and behind the Schur complement, ...
  double* chiE;                         // [nChi] visual edges, links, the two priors
  LmControl* lm;
  double* chi2;                         // [2]
  int* lmi;                             // [8] LMW_* (lm_control.h)
  int* lmHost;                          // mapped host words: [0] decided trials, [1] done, [2] the caller's stop flag as the host forwards it
  double priorG, priorA;
  CamGeom g;
};

__device__ __forceinline__ void fiba_load(const CamGeom& g, const double* s, VIState& V) {
  for (int k = 0; k < 9; ++k) { V.Rwb[k] = s[k]; V.Rcw[k] = s[21 + k]; }
  for (int k = 0; k < 3; ++k) { V.twb[k] = s[9 + k]; V.v[k] = s[12 + k]; V.bg[k] = s[15 + k]; V.ba[k] = s[18 + k]; V.tcw[k] = s[30 + k]; }
  if (g.rig) refresh_camera(g, V);   // the right camera's pose is derived, not stored
}
template <bool RIG>
__device__ __forceinline__ void fiba_load_t(const CamGeom& g, const double* s, VIState& V) {   // RIG as a template parameter keeps the right camera out of the pinhole form's registers
  for (int k = 0; k < 9; ++k) { V.Rwb[k] = s[k]; V.Rcw[k] = s[21 + k]; }
  for (int k = 0; k < 3; ++k) { V.twb[k] = s[9 + k]; V.v[k] = s[12 + k]; V.bg[k] = s[15 + k]; V.ba[k] = s[18 + k]; V.tcw[k] = s[30 + k]; }
  if (RIG) refresh_camera_t<true>(g, V);
}
__device__ __forceinline__ void fiba_load_imu(const double* s, VIState& V) {   // what a link reads
  for (int k = 0; k < 9; ++k) V.Rwb[k] = s[k];
  for (int k = 0; k < 3; ++k) { V.twb[k] = s[9 + k]; V.v[k] = s[12 + k]; V.bg[k] = s[15 + k]; V.ba[k] = s[18 + k]; }
}
__device__ __forceinline__ void fiba_store(const VIState& V, double* s) {
  for (int k = 0; k < 9; ++k) { s[k] = V.Rwb[k]; s[21 + k] = V.Rcw[k]; }
  for (int k = 0; k < 3; ++k) { s[9 + k] = V.twb[k]; s[12 + k] = V.v[k]; s[15 + k] = V.bg[k]; s[18 + k] = V.ba[k]; s[30 + k] = V.tcw[k]; }
}
// 3 x 3 inverse by Gauss-Jordan with partial pivoting, the oracle's steps one by one: a point seen through one monocular edge has a block
// of rank 2 + lambda, and at lambda = 1e-5 a cofactor inverse loses what the Schur complement's cancellation then needs.  Rows are
// exchanged by name, not by index: everything stays in registers.  A zero pivot: the zero matrix.
__device__ __forceinline__ void fiba_swap_rows(double* a, double* b) {
#pragma unroll
  for (int k = 0; k < 6; ++k) { const double t = a[k]; a[k] = b[k]; b[k] = t; }
}
__device__ __forceinline__ void fiba_inv3(const double* m, double* o) {
  double r0[6] = {m[0], m[1], m[2], 1, 0, 0}, r1[6] = {m[3], m[4], m[5], 0, 1, 0}, r2[6] = {m[6], m[7], m[8], 0, 0, 1};
  bool ok = true;
  // column 0
  {
    int p = 0;
    if (fabs(r1[0]) > fabs(r0[0])) p = 1;
    if (fabs(r2[0]) > fabs(p ? r1[0] : r0[0])) p = 2;
    if (p == 1) fiba_swap_rows(r0, r1);
    if (p == 2) fiba_swap_rows(r0, r2);
    ok = ok && r0[0] != 0.0;
    const double inv = 1.0 / r0[0];
#pragma unroll
    for (int k = 0; k < 6; ++k) r0[k] *= inv;
    const double f1 = r1[0], f2 = r2[0];
#pragma unroll
    for (int k = 0; k < 6; ++k) { if (f1 != 0.0) r1[k] -= f1 * r0[k]; if (f2 != 0.0) r2[k] -= f2 * r0[k]; }
  }
  // column 1
  {
    if (fabs(r2[1]) > fabs(r1[1])) fiba_swap_rows(r1, r2);
    ok = ok && r1[1] != 0.0;
    const double inv = 1.0 / r1[1];
#pragma unroll
    for (int k = 0; k < 6; ++k) r1[k] *= inv;
    const double f0 = r0[1], f2 = r2[1];
#pragma unroll
    for (int k = 0; k < 6; ++k) { if (f0 != 0.0) r0[k] -= f0 * r1[k]; if (f2 != 0.0) r2[k] -= f2 * r1[k]; }
  }
  // column 2
  {
    ok = ok && r2[2] != 0.0;
    const double inv = 1.0 / r2[2];
#pragma unroll
    for (int k = 0; k < 6; ++k) r2[k] *= inv;
    const double f0 = r0[2], f1 = r1[2];
#pragma unroll
    for (int k = 0; k < 6; ++k) { if (f0 != 0.0) r0[k] -= f0 * r2[k]; if (f1 != 0.0) r1[k] -= f1 * r2[k]; }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { o[k] = ok ? r0[3 + k] : 0.0; o[3 + k] = ok ? r1[3 + k] : 0.0; o[6 + k] = ok ? r2[3 + k] : 0.0; }
}
__device__ __forceinline__ double fiba_quad(const double* e, const double* Om, int n) {
  double s = 0;
  for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) s += e[r] * Om[r * n + c] * e[c];
  return s;
}
__device__ __forceinline__ bool fiba_stop(const FibaDev& D) { return __hip_atomic_load(D.lmHost + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0; }
__device__ __forceinline__ double fiba_delta_mono() { return (double)(float)sqrt(5.991); }
__device__ __forceinline__ double fiba_delta_stereo() { return (double)(float)sqrt(7.815); }
// the biases a link is evaluated at: keyframe 1's own, or the map's shared ones (:464-472)
__device__ __forceinline__ void fiba_link_bias(const FibaDev& D, const double* sb, VIState& V1) {
  if (!D.bInit) return;
  for (int k = 0; k < 3; ++k) { V1.bg[k] = sb[k]; V1.ba[k] = sb[3 + k]; }
}

// the caller's floats to FP64 states (with the camera poses of ImuCamPose), points and shared biases
__global__ __launch_bounds__(FIBA_NT) void k_fiba_setup(FibaDev D) {
  const int t = blockIdx.x * FIBA_NT + threadIdx.x;
  if (t < D.nKF) {
    VIState V;
    load_state(D.g, D.kfIn + 21 * (size_t)t, V);
    fiba_store(V, D.S + 33 * (size_t)t);
  }
  if (t < 3 * D.nMP) D.pt[t] = (double)D.mpIn[t];
  if (t < 6) D.sb[t] = D.bInit ? (double)D.biasIn[t] : 0.0;
}

// computeError and the robust chi2 of every edge at the trial estimate (trial != 0) or at the current one: visual edges, links (EdgeInertial
// under Huber, EdgeGyroRW, EdgeAccRW), the two priors
__global__ __launch_bounds__(FIBA_NT) void k_fiba_errors(FibaDev D, int trial) {
  if (D.lmi[LMW_DONE]) return;
  const int t = blockIdx.x * FIBA_NT + threadIdx.x;
  if (t >= D.nChi) return;
  const double *S = trial ? D.ST : D.S, *pt = trial ? D.ptT : D.pt, *sb = trial ? D.sbT : D.sb;
  double w, c;
  if (t < D.nE) {
    VIState V;
    fiba_load(D.g, S + 33 * (size_t)D.eKF[t], V);
    const float* o = D.eObs + 3 * (size_t)t;
    const bool st = !D.g.rig && !(o[2] < 0);
    const double* Xp = pt + 3 * (size_t)D.eMP[t];
    const double X[3] = {Xp[0], Xp[1], Xp[2]};
    double err[3], Xc[3];
    const double chi = vis_error(D.g, V, X, o, st, (double)D.eInfo[t], err, Xc, D.eRight && D.eRight[t] ? 1 : 0);
    c = huber(st ? fiba_delta_stereo() : fiba_delta_mono(), chi, &w);
  } else if (t < D.nE + D.nI) {
    const int i = t - D.nE;
    VIState V1, V2;
    fiba_load_imu(S + 33 * (size_t)D.iKF1[i], V1);
    fiba_load_imu(S + 33 * (size_t)D.iKF2[i], V2);
    double ge[3] = {0, 0, 0}, ae[3] = {0, 0, 0}, err[9];
    if (!D.bInit) for (int k = 0; k < 3; ++k) { ge[k] = V2.bg[k] - V1.bg[k]; ae[k] = V2.ba[k] - V1.ba[k]; }   // EdgeGyroRW, EdgeAccRW
    fiba_link_bias(D, sb, V1);
    inertial_edge(D.iPre[i], V1, V2, nullptr, true, err, nullptr);
    c = huber(sqrt(16.92), fiba_quad(err, D.InfoI + (size_t)i * 81, 9), &w);
    if (!D.bInit) c += fiba_quad(ge, D.InfoG + (size_t)i * 9, 3) + fiba_quad(ae, D.InfoA + (size_t)i * 9, 3);
  } else {   // EdgePriorGyro, EdgePriorAcc: e = 0 - bias, information prior * I
    const int a = t - D.nE - D.nI;
    const double* e = sb + 3 * a;
    const double pr = a ? D.priorA : D.priorG;
    c = e[0] * pr * e[0] + e[1] * pr * e[1] + e[2] * pr * e[2];
  }
  D.chiE[t] = c;
}

// linearizeOplus and the robust weight of every visual edge at the current estimate
template <bool RIG>
__global__ __launch_bounds__(FIBA_NT) void k_fiba_linearize(FibaDev D) {
  if (D.lmi[LMW_DONE] || !D.lmi[LMW_REBUILD]) return;
  const int e = blockIdx.x * FIBA_NT + threadIdx.x;
  if (e >= D.nE) return;
  VIState V;
  fiba_load_t<RIG>(D.g, D.S + 33 * (size_t)D.eKF[e], V);
  const float* o = D.eObs + 3 * (size_t)e;
  const bool st = !RIG && !(o[2] < 0);
  const int cam = RIG && D.eRight[e] ? 1 : 0;
  const double info = (double)D.eInfo[e];
  const double* Xp = D.pt + 3 * (size_t)D.eMP[e];
  const double X[3] = {Xp[0], Xp[1], Xp[2]};
  double err[3], Xc[3], w, Jp[18], Jl[9], pj[9], Rc[9];
  const double chi = vis_error_t<RIG>(D.g, V, X, o, st, info, err, Xc, cam);
  huber(st ? fiba_delta_stereo() : fiba_delta_mono(), chi, &w);
  vis_jacobian_t<RIG>(D.g, Xc, st, Jp, cam);
  cam_project_jac_t<RIG>(D.g, Xc, cam, pj);
  pj[6] = pj[7] = pj[8] = 0;
  if (st) { pj[6] = pj[0]; pj[7] = pj[1]; pj[8] = pj[2] + D.g.bf * (1.0 / (Xc[2] * Xc[2])); }
#pragma unroll
  for (int r = 0; r < 9; ++r) Rc[r] = (RIG && cam) ? V.Rcw1[r] : V.Rcw[r];   // (element-wise selects, as k_iba_kf)
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) Jl[r * 3 + c] = -(pj[r * 3] * Rc[c] + pj[r * 3 + 1] * Rc[3 + c] + pj[r * 3 + 2] * Rc[6 + c]);
  double* out = D.E + (size_t)e * FIBA_EDGE;
#pragma unroll
  for (int k = 0; k < 18; ++k) out[FE_JP + k] = Jp[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) out[FE_JL + k] = Jl[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) out[FE_RW + k] = -info * err[k] * w;
  out[FE_WO] = w * info;
}

// a link's record: one wave per link; lane 0 evaluates EdgeInertial (error, 9 x 24 Jacobian) into LDS, all lanes multiply out
__global__ __launch_bounds__(64) void k_fiba_links(FibaDev D) {
  __shared__ double J[216], OJ[216], Oe[9], ge[3], ae[3];
  __shared__ double sw;
  if (D.lmi[LMW_DONE] || !D.lmi[LMW_REBUILD]) return;
  const int i = blockIdx.x, tid = threadIdx.x;
  for (int k = tid; k < 216; k += 64) J[k] = 0;
  __syncthreads();
  const double* Om = D.InfoI + (size_t)i * 81;
  if (tid == 0) {
    VIState V1, V2;
    fiba_load_imu(D.S + 33 * (size_t)D.iKF1[i], V1);
    fiba_load_imu(D.S + 33 * (size_t)D.iKF2[i], V2);
    for (int k = 0; k < 3; ++k) { ge[k] = D.bInit ? 0.0 : V2.bg[k] - V1.bg[k]; ae[k] = D.bInit ? 0.0 : V2.ba[k] - V1.ba[k]; }   // (no random-walk edges with bInit)
    fiba_link_bias(D, D.sb, V1);
    double err[9], w;
    inertial_edge(D.iPre[i], V1, V2, nullptr, true, err, J);
    huber(sqrt(16.92), fiba_quad(err, Om, 9), &w);
    sw = w;
    for (int r = 0; r < 9; ++r) { double sm = 0; for (int l = 0; l < 9; ++l) sm += Om[r * 9 + l] * err[l]; Oe[r] = sm; }
  }
  __syncthreads();
  for (int k = tid; k < 216; k += 64) { const int r = k / 24, c = k - r * 24; double sm = 0; for (int l = 0; l < 9; ++l) sm += Om[r * 9 + l] * J[l * 24 + c]; OJ[k] = sm; }
  __syncthreads();
  const double w = sw;
  const double *Qg = D.InfoG + (size_t)i * 9, *Qa = D.InfoA + (size_t)i * 9;
  double* out = D.LR + (size_t)i * FIBA_LREC;
  // the random-walk edges sit on the bias columns: 9 .. 14 of keyframe 1, 24 .. 29 of keyframe 2; type 0 gyro, 1 accelerometer
  auto rw_of = [](int a, int* type, int* side, int* row) {
    const int q = a >= 24 ? a - 24 : a - 9;
    if (a < 9 || (a >= 15 && a < 24)) { *type = -1; return; }
    *type = q / 3; *row = q % 3; *side = a >= 24 ? 1 : 0;
  };
  for (int idx = tid; idx < FIBA_LREC; idx += 64) {
    double v = 0;
    if (idx < FIBA_LCOLS * FIBA_LCOLS) {
      const int a = idx / FIBA_LCOLS, b2 = idx - a * FIBA_LCOLS;
      if (a < 24 && b2 < 24) {
        double h = 0;
        for (int k = 0; k < 9; ++k) h += J[k * 24 + a] * OJ[k * 24 + b2];
        v = w * h;
      }
      if (!D.bInit) {
        int ta, sa, ra, tb, sb2, rb;
        rw_of(a, &ta, &sa, &ra); rw_of(b2, &tb, &sb2, &rb);
        if (ta >= 0 && ta == tb) { const double q = (ta ? Qa : Qg)[ra * 3 + rb]; v += sa == sb2 ? q : -q; }
      }
    } else {
      const int a = idx - FIBA_LCOLS * FIBA_LCOLS;
      if (a < 24) {
        double sm = 0;
        for (int k = 0; k < 9; ++k) sm += J[k * 24 + a] * Oe[k];
        v = -w * sm;
      }
      if (!D.bInit) {
        int ta, sa, ra;
        rw_of(a, &ta, &sa, &ra);
        if (ta >= 0) {   // e = bias 2 - bias 1: -Q e on keyframe 2, +Q e on keyframe 1
          const double* Q = ta ? Qa : Qg;
          const double* e3 = ta ? ae : ge;
          const double sm = Q[ra * 3] * e3[0] + Q[ra * 3 + 1] * e3[1] + Q[ra * 3 + 2] * e3[2];
          v += sa ? -sm : sm;
        }
      }
    }
    out[idx] = v;
  }
}

// sum over the edges list[k0 .. k1) of (A^T wo B)(r, c), A = the record's Jacobian at offset oa with sa columns, B likewise; in edge order
__device__ __forceinline__ double fiba_sum_jtj(const double* E, const int* list, int k0, int k1, int oa, int sa, int r, int ob, int sb, int c) {
  double acc = 0;
  for (int k = k0; k < k1; ++k) {
    const double* rec = E + (size_t)list[k] * FIBA_EDGE;
    const double wo = rec[FE_WO];
    double h = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) h += rec[oa + i * sa + r] * wo * rec[ob + i * sb + c];
    acc += h;
  }
  return acc;
}
__device__ __forceinline__ double fiba_sum_jtr(const double* E, const int* list, int k0, int k1, int oa, int sa, int r) {
  double acc = 0;
  for (int k = k0; k < k1; ++k) {
    const double* rec = E + (size_t)list[k] * FIBA_EDGE;
    double s = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) s += rec[oa + i * sa + r] * rec[FE_RW + i];
    acc += s;
  }
  return acc;
}

// Hpp, bp (42 lanes per keyframe of the system), Hll, bl (12 per point), Hpl (18 per pair)
__global__ __launch_bounds__(FIBA_NT) void k_fiba_assemble(FibaDev D) {
  if (D.lmi[LMW_DONE] || !D.lmi[LMW_REBUILD]) return;
  size_t gid = (size_t)blockIdx.x * FIBA_NT + threadIdx.x;
  if (gid < (size_t)D.nSys * 42) {
    const int a = (int)(gid / 42), k = (int)(gid % 42);
    const int k0 = D.kfStart[a], k1 = D.kfStart[a + 1];
    if (k < 36) D.Hpp[(size_t)a * 36 + k] = fiba_sum_jtj(D.E, D.kfEdges, k0, k1, FE_JP, 6, k / 6, FE_JP, 6, k % 6);
    else D.bp[(size_t)a * 6 + k - 36] = fiba_sum_jtr(D.E, D.kfEdges, k0, k1, FE_JP, 6, k - 36);
    return;
  }
  gid -= (size_t)D.nSys * 42;
  if (gid < (size_t)D.nMP * 12) {
    const int m = (int)(gid / 12), k = (int)(gid % 12);
    const int k0 = D.mpStart[m], k1 = D.mpStart[m + 1];
    if (k < 9) D.Hll[(size_t)m * 9 + k] = fiba_sum_jtj(D.E, D.mpEdges, k0, k1, FE_JL, 3, k / 3, FE_JL, 3, k % 3);
    else D.bl[(size_t)m * 3 + k - 9] = fiba_sum_jtr(D.E, D.mpEdges, k0, k1, FE_JL, 3, k - 9);
    return;
  }
  gid -= (size_t)D.nMP * 12;
  if (gid < (size_t)D.nPairs * 18) {
    const int p = (int)(gid / 18), k = (int)(gid % 18);
    D.Hpl[gid] = fiba_sum_jtj(D.E, D.pairEdges, D.pairStart[p], D.pairStart[p + 1], FE_JP, 6, k / 3, FE_JL, 3, k % 3);
  }
}

// Dinv per point; Hpl Dinv and Hpl Dinv bl per pair (a pair's lane inverts its point's block itself)
__global__ __launch_bounds__(FIBA_NT) void k_fiba_dinv(FibaDev D) {
  if (D.lmi[LMW_DONE]) return;
  const int gid = blockIdx.x * FIBA_NT + threadIdx.x;
  if (gid >= D.nMP + D.nPairs) return;
  const double lambda = D.lm->lambda;
  const int p = gid - D.nMP, m = gid < D.nMP ? gid : D.pairMp[p];
  double Hl[9], Di[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Hl[k] = D.Hll[(size_t)m * 9 + k];
  Hl[0] += lambda; Hl[4] += lambda; Hl[8] += lambda;
  fiba_inv3(Hl, Di);
  if (gid < D.nMP) {
    const bool has = D.mpStart[m + 1] > D.mpStart[m];
#pragma unroll
    for (int k = 0; k < 9; ++k) D.Dinv[(size_t)m * 9 + k] = has ? Di[k] : 0.0;
    return;
  }
  const double* W = D.Hpl + (size_t)p * 18;
  const double* bl = D.bl + (size_t)m * 3;
  double db[3];   // Dinv bl
#pragma unroll
  for (int j = 0; j < 3; ++j) db[j] = Di[j * 3] * bl[0] + Di[j * 3 + 1] * bl[1] + Di[j * 3 + 2] * bl[2];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) D.HplD[(size_t)p * 18 + i * 3 + j] = W[i * 3] * Di[j] + W[i * 3 + 1] * Di[3 + j] + W[i * 3 + 2] * Di[6 + j];
    D.hg[(size_t)p * 6 + i] = W[i * 3] * db[0] + W[i * 3 + 1] * db[1] + W[i * 3 + 2] * db[2];
  }
}

// a chunk of an envelope block's contributions: sum of (Hpl_i1 Dinv) Hpl_i2^T restricted to the block, a lane per (chunk, entry), in point order
__global__ __launch_bounds__(FIBA_NT) void k_fiba_schur(FibaDev D) {
  if (D.lmi[LMW_DONE]) return;
  const size_t gid = (size_t)blockIdx.x * FIBA_NT + threadIdx.x;
  if (gid >= (size_t)D.nChunks * 9) return;
  const int c = (int)(gid / 9), ent = (int)(gid % 9), r = ent / 3, cc = ent % 3;
  double acc = 0;
  for (int q = D.chunkStart[c]; q < D.chunkEnd[c]; ++q) {
    const int2 pr = D.ct[q];
    const double* A = D.HplD + (size_t)(pr.x >> 1) * 18 + ((pr.x & 1) * 3 + r) * 3;
    const double* B = D.Hpl + (size_t)(pr.y >> 1) * 18 + ((pr.y & 1) * 3 + cc) * 3;
    acc += A[0] * B[0] + A[1] * B[1] + A[2] * B[2];
  }
  D.part[gid] = acc;
}

// the reduced system: an envelope entry = the keyframe's visual block + its links' records in link order + the prior - the chunks' sums in
// order; a row of b likewise, minus sum Hpl Dinv bl over the keyframe's pairs in point order
__global__ __launch_bounds__(FIBA_NT) void k_fiba_finish(FibaDev D) {
  if (D.lmi[LMW_DONE]) return;
  const size_t gid = (size_t)blockIdx.x * FIBA_NT + threadIdx.x;
  const size_t nH = (size_t)D.nBlocks * 9;
  if (gid < nH) {
    const int blk = (int)(gid / 9), ent = (int)(gid % 9), r = ent / 3, c = ent % 3;
    double acc = 0;
    for (int q = D.blkChunkStart[blk]; q < D.blkChunkStart[blk + 1]; ++q) acc += D.part[(size_t)q * 9 + ent];
    double base = 0;
    const int v = D.blkVis[blk];
    if (v >= 0) {
      const int hr = (v & 3) ? 1 : 0, hc = (v & 3) == 2 ? 1 : 0;
      base = D.Hpp[(size_t)(v >> 2) * 36 + (3 * hr + r) * 6 + 3 * hc + c];
    }
    for (int q = D.blkLinkStart[blk]; q < D.blkLinkStart[blk + 1]; ++q) {
      const int it = D.blkLinks[q];
      base += D.LR[(size_t)(it >> 8) * FIBA_LREC + (3 * ((it >> 4) & 15) + r) * FIBA_LCOLS + 3 * (it & 15) + c];
    }
    const int a = D.blkDiag[blk];
    if (D.bInit && r == c && a >= D.rbB) base += a == D.rbB ? D.priorG : D.priorA;
    D.H[gid] = base - acc;
    return;
  }
  const size_t k = gid - nH;
  if (k >= (size_t)D.P) return;
  const int br = (int)(k / 3), r = (int)(k % 3);
  double base = 0, acc = 0;
  const int v = D.rowVis[br];
  if (v >= 0) {
    const int a = v >> 1, rr = 3 * (v & 1) + r;
    base = D.bp[(size_t)a * 6 + rr];
    for (int q = D.kfPairStart[a]; q < D.kfPairStart[a + 1]; ++q) acc += D.hg[(size_t)D.kfPairs[q] * 6 + rr];
  }
  for (int q = D.rowLinkStart[br]; q < D.rowLinkStart[br + 1]; ++q) {
    const int it = D.rowLinks[q];
    base += D.LR[(size_t)(it >> 4) * FIBA_LREC + FIBA_LCOLS * FIBA_LCOLS + 3 * (it & 15) + r];
  }
  if (D.bInit && br >= D.rbB) base += -(br == D.rbB ? D.priorG : D.priorA) * D.sb[3 * (br - D.rbB) + r];   // e = 0 - bias, d e / d bias = -I
  D.b0[k] = base;
  D.b[k] = base - acc;
}

// H + lambda I = L D L^T over the envelope, and y = L^-1 b on the way (envelope_ldlt.h).  One workgroup.  A zero or NaN pivot fails.
__global__ __launch_bounds__(FIBA_NT) void k_fiba_factor(FibaDev D) {
  if (D.lmi[LMW_DONE]) return;
  const bool ok = envelope_factor<3, FIBA_NT, FIBA_STAGE, 1, false>(envelope_sys(D), D.lm->lambda);
  if (threadIdx.x == 0) D.lmi[LMW_OK2] = ok ? 1 : 0;
}

// x = L^-T D^-1 y (envelope_ldlt.h), then the trial states: ImuCamPose::Update for the pose, additive velocity and biases, the shared
// biases once.  One workgroup.  A failed factorisation leaves the step zero.
__global__ __launch_bounds__(FIBA_NT) void k_fiba_backsub(FibaDev D) {
  if (D.lmi[LMW_DONE]) return;
  const int t = threadIdx.x, n = D.n;
  if (D.lmi[LMW_OK2]) {
    envelope_backsub<3, FIBA_NT>(envelope_sys(D));
  } else {
    for (int i = t; i < 3 * n; i += FIBA_NT) D.x[i] = 0.0;
    __threadfence_block();
    __syncthreads();
  }
  for (int v = t; v < D.nKF; v += FIBA_NT) {
    const int o = D.off[v];
    if (o < 0) {
      for (int k = 0; k < 33; ++k) D.ST[33 * (size_t)v + k] = D.S[33 * (size_t)v + k];
      continue;
    }
    VIState V;
    fiba_load(D.g, D.S + 33 * (size_t)v, V);
    const int w = D.wid[v];
    double dx[15];
#pragma unroll
    for (int q = 0; q < 15; ++q) dx[q] = q < w ? D.x[o + (q < w ? q : 0)] : 0.0;
    apply_update(D.g, V, dx);
    fiba_store(V, D.ST + 33 * (size_t)v);
  }
  if (t < 6) D.sbT[t] = D.sb[t] + (D.bInit ? D.x[D.P - 6 + t] : 0.0);
}

// xl = Dinv (bl - Hpl^T xp) over the point's pairs in order, and the trial points
__global__ __launch_bounds__(FIBA_NT) void k_fiba_points(FibaDev D) {
  if (D.lmi[LMW_DONE]) return;
  const int m = blockIdx.x * FIBA_NT + threadIdx.x;
  if (m >= D.nMP) return;
  double xl[3] = {0, 0, 0};
  if (D.lmi[LMW_OK2] && D.mpStart[m + 1] > D.mpStart[m]) {
    double cl[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) cl[j] = D.bl[(size_t)m * 3 + j];
    for (int p = D.mpPairStart[m]; p < D.mpPairStart[m + 1]; ++p) {
      const double* W = D.Hpl + (size_t)p * 18;
      const double* xp = D.x + D.pairOff[p];
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

// init != 0: behind the first computeActiveErrors; else g2o's decision after a trial (lm_control.h).  One workgroup.
__global__ __launch_bounds__(FIBA_NT) void k_fiba_decide(FibaDev D, int init) {
  __shared__ double buf[FIBA_NT];
  __shared__ int sKeep;
  if (D.lmi[LMW_DONE]) return;
  const int t = threadIdx.x;
  const double chi = lm_sum_of_lane_slices<FIBA_NT>(buf, D.nChi, [&](int e) { return D.chiE[e]; });
  LmControl c = *D.lm;
  if (init) {
    if (t == 0) {
      const int stop = fiba_stop(D) ? 1 : 0;   // (raised between the entry and the first iteration: optimize() ends before it)
      lm_begin(c, 1e-5, 0.0);                  // setUserLambdaInit(1e-5) (:384)
      lm_iteration(c, chi);
      *D.lm = c;
      D.chi2[0] = chi; D.chi2[1] = chi;
      D.lmi[LMW_REBUILD] = 1; D.lmi[LMW_ITS] = 0; D.lmi[LMW_TRIALS] = 0; D.lmi[LMW_OK2] = 1; D.lmi[LMW_DONE] = stop;
      if (stop) __hip_atomic_store(D.lmHost + 1, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return;
  }
  const double lambda = c.lambda;
  const double gainP = lm_sum_of_lane_slices<FIBA_NT>(buf, D.P, [&](int i) { return D.x[i] * (lambda * D.x[i] + D.b0[i]); });   // computeScale()
  const double gainL = lm_sum_of_lane_slices<FIBA_NT>(buf, 3 * D.nMP, [&](int i) { return D.xl[i] * (lambda * D.xl[i] + D.bl[i]); });
  if (t == 0) sKeep = lm_decide_trial(c, chi, D.lmi[LMW_OK2] != 0, gainP + gainL, fiba_stop(D), D.maxIts, D.lm, D.chi2, D.lmi, D.lmHost) ? 1 : 0;
  __syncthreads();
  if (sKeep) {
    for (int i = t; i < 33 * D.nKF; i += FIBA_NT) D.S[i] = D.ST[i];
    for (int i = t; i < 3 * D.nMP; i += FIBA_NT) D.pt[i] = D.ptT[i];
    if (t < 6) D.sb[t] = D.sbT[t];
  }
}

// ---- the host's part ----

// n x n inverse by Gauss-Jordan with partial pivoting
bool fiba_invert(const double* A, int n, double* Ainv) {
  std::vector<double> M((size_t)n * 2 * n, 0.0);
  const int w = 2 * n;
  for (int r = 0; r < n; ++r) { for (int c = 0; c < n; ++c) M[(size_t)r * w + c] = A[r * n + c]; M[(size_t)r * w + n + r] = 1.0; }
  for (int c = 0; c < n; ++c) {
    int p = c;
    for (int r = c + 1; r < n; ++r) if (std::fabs(M[(size_t)r * w + c]) > std::fabs(M[(size_t)p * w + c])) p = r;
    if (M[(size_t)p * w + c] == 0.0) return false;
    if (p != c) for (int k = 0; k < w; ++k) std::swap(M[(size_t)p * w + k], M[(size_t)c * w + k]);
    const double inv = 1.0 / M[(size_t)c * w + c];
    for (int k = 0; k < w; ++k) M[(size_t)c * w + k] *= inv;
    for (int r = 0; r < n; ++r) {
      const double f = M[(size_t)r * w + c];
      if (r != c && f != 0.0) for (int k = 0; k < w; ++k) M[(size_t)r * w + k] -= f * M[(size_t)c * w + k];
    }
  }
  for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) Ainv[r * n + c] = M[(size_t)r * w + n + c];
  return true;
}
// EdgeInertial's information (G2oTypes.cc:484-491): C(0:9, 0:9)^-1, symmetrised, eigenvalues below 1e-12 set to zero (cyclic Jacobi).  Once
// per link and call, on the host.
void fiba_inertial_information(const float* C15, double* Info) {
  double C9[81], Inv[81], a[81], V[81];
  for (int r = 0; r < 9; ++r) for (int c = 0; c < 9; ++c) C9[r * 9 + c] = (double)C15[r * 15 + c];
  if (!fiba_invert(C9, 9, Inv)) { memset(Info, 0, sizeof(double) * 81); return; }
  const int n = 9;
  for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) { a[r * n + c] = (Inv[r * n + c] + Inv[c * n + r]) / 2; V[r * n + c] = r == c ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0, diag = 0;
    for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) (r == c ? diag : off) += a[r * n + c] * a[r * n + c];
    if (off <= 1e-30 * diag) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        if (a[p * n + q] == 0.0) continue;
        const double theta = (a[q * n + q] - a[p * n + p]) / (2.0 * a[p * n + q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) { const double x = a[k * n + p], y = a[k * n + q]; a[k * n + p] = c * x - s * y; a[k * n + q] = s * x + c * y; }
        for (int k = 0; k < n; ++k) { const double x = a[p * n + k], y = a[q * n + k]; a[p * n + k] = c * x - s * y; a[q * n + k] = s * x + c * y; }
        for (int k = 0; k < n; ++k) { const double x = V[k * n + p], y = V[k * n + q]; V[k * n + p] = c * x - s * y; V[k * n + q] = s * x + c * y; }
      }
  }
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) {
      double s = 0;
      for (int k = 0; k < n; ++k) s += V[r * n + k] * (a[k * n + k] < 1e-12 ? 0.0 : a[k * n + k]) * V[c * n + k];
      Info[r * n + c] = s;
    }
}

bool fiba_finite(const float* p, size_t n) {
  for (size_t k = 0; k < n; ++k) if (!std::isfinite(p[k])) return false;
  return true;
}

int fiba_run(morb_optimizer* o, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos, int nE, const int* eKF, const int* eMP,
             const float* eObs, const uint8_t* eRight, const float* eInvSigma2, int nI, const int* iKF1, const int* iKF2,
             const morb_imu_preintegrated* iPre, const float* cam5, const float* rig28, const float* Tbc12, int its, int bInit, float priorG,
             float priorA, float* bias6, const uint8_t* pbStopFlag, int* stats4, double* chi2) {
  MORB_REQUIRE(o && kfState21 && kfKind && mpPos && eKF && eMP && eObs && eInvSigma2 && Tbc12 && stats4 && chi2, MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nI == 0 || (iKF1 && iKF2 && iPre), MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(!bInit || bias6, MORB_ERR_INVALID, "bias6 is NULL with bInit");
  MORB_REQUIRE(nKF > 0 && nMP > 0 && nE > 0 && nI >= 0, MORB_ERR_INVALID, "empty problem");
  MORB_REQUIRE(its >= 1 && its <= 100, MORB_ERR_INVALID, "its outside 1 .. 100");
  bInit = bInit ? 1 : 0;
  for (int k = 0; k < nKF; ++k) MORB_REQUIRE(kfKind[k] <= 3, MORB_ERR_INVALID, "kfKind out of range");
  MORB_REQUIRE(fiba_finite(kfState21, (size_t)21 * nKF) && fiba_finite(mpPos, (size_t)3 * nMP), MORB_ERR_INVALID, "a non-finite state or point");
  MORB_REQUIRE(fiba_finite(eObs, (size_t)3 * nE) && fiba_finite(eInvSigma2, nE), MORB_ERR_INVALID, "a non-finite observation or information");
  MORB_REQUIRE(fiba_finite(Tbc12, 12) && (!cam5 || fiba_finite(cam5, 5)) && (!rig28 || fiba_finite(rig28, 28)), MORB_ERR_INVALID, "a non-finite calibration");
  MORB_REQUIRE(fiba_finite((const float*)iPre, (size_t)nI * (sizeof(morb_imu_preintegrated) / sizeof(float))), MORB_ERR_INVALID, "a non-finite preintegration");
  if (bInit) MORB_REQUIRE(fiba_finite(bias6, 6) && std::isfinite(priorG) && std::isfinite(priorA), MORB_ERR_INVALID, "a non-finite bias or prior");
  for (int e = 0; e < nE; ++e) MORB_REQUIRE(eKF[e] >= 0 && eKF[e] < nKF && eMP[e] >= 0 && eMP[e] < nMP, MORB_ERR_INVALID, "edge index out of range");
  std::vector<char> linked(nKF, 0);
  for (int i = 0; i < nI; ++i) {
    MORB_REQUIRE(iKF1[i] >= 0 && iKF1[i] < nKF && iKF2[i] >= 0 && iKF2[i] < nKF && iKF1[i] != iKF2[i], MORB_ERR_INVALID, "link index out of range");
    MORB_REQUIRE(kfKind[iKF1[i]] <= 1 && kfKind[iKF2[i]] <= 1, MORB_ERR_INVALID, "link ends on a keyframe without velocity and biases");
    linked[iKF1[i]] = linked[iKF2[i]] = 1;
  }
  for (int k = 0; k < nKF; ++k) MORB_REQUIRE(kfKind[k] != 0 || linked[k], MORB_ERR_INVALID, "a keyframe of kind 0 enters no link: pass it as kind 3");
  // ---- the symbolic pass: the keyframes of the system and their rows, the (point, keyframe) pairs, the envelope, the contribution lists ----
  std::vector<char> seen(nKF, 0);
  for (int e = 0; e < nE; ++e) seen[eKF[e]] = 1;
  std::vector<int> off(nKF, -1), wid(nKF, 0), sysIdx(nKF, -1), sysKF;
  int P = 0;
  for (int k = 0; k < nKF; ++k) {
    const int w = kfKind[k] == 0 ? (bInit ? 9 : 15) : (kfKind[k] == 3 && seen[k]) ? 6 : 0;
    if (!w) continue;
    sysIdx[k] = (int)sysKF.size(); sysKF.push_back(k); off[k] = P; wid[k] = w; P += w;
  }
  const int nSys = (int)sysKF.size();
  auto nothing = [&]() {   // no keyframe is in the system: nothing to optimise, nothing written
    for (int k = 0; k < 4; ++k) stats4[k] = 0;
    chi2[0] = chi2[1] = 0;
    return MORB_OK;
  };
  if (!nSys) return nothing();
  const int rbB = bInit ? P / 3 : -1;
  if (bInit) P += 6;
  const int n = P / 3;
  std::vector<int> mpStart, mpEdges;
  csr_by_key(eMP, nE, nMP, mpStart, mpEdges);
  std::vector<int> pairKF, pairMp, pairStart, pairEdges, mpPairStart(nMP + 1, 0);
  std::vector<int> firstKf(nSys);   // the lowest keyframe of the system a keyframe shares a point or a link with
  for (int a = 0; a < nSys; ++a) firstKf[a] = a;
  size_t nCt = 0;
  {
    std::vector<std::pair<int, int>> ke;
    for (int m = 0; m < nMP; ++m) {
      ke.clear();
      for (int k = mpStart[m]; k < mpStart[m + 1]; ++k) if (off[eKF[mpEdges[k]]] >= 0) ke.push_back({eKF[mpEdges[k]], mpEdges[k]});
      std::sort(ke.begin(), ke.end());
      for (size_t k = 0; k < ke.size(); ++k) {
        if (k == 0 || ke[k].first != ke[k - 1].first) {
          pairStart.push_back((int)pairEdges.size());
          pairKF.push_back(ke[k].first); pairMp.push_back(m);
          int& f = firstKf[sysIdx[ke[k].first]];
          f = std::min(f, sysIdx[ke[0].first]);
        }
        pairEdges.push_back(ke[k].second);
      }
      mpPairStart[m + 1] = (int)pairKF.size();
      const size_t k = (size_t)(mpPairStart[m + 1] - mpPairStart[m]);
      nCt += 4 * (k * (k + 1) / 2) - k;   // four 3 x 3 blocks per keyframe pair, three on the diagonal
    }
    pairStart.push_back((int)pairEdges.size());
  }
  const int nPairs = (int)pairKF.size();
  MORB_REQUIRE(nCt <= (size_t)INT_MAX, MORB_ERR_CAPACITY, "more Schur pair contributions than an int indexes");
  int firstShared = nSys;   // the shared biases' rows begin at the lowest keyframe of the system that enters a link
  for (int i = 0; i < nI; ++i) {
    const int a = sysIdx[iKF1[i]], b = sysIdx[iKF2[i]];
    if (a >= 0 && b >= 0) { firstKf[std::max(a, b)] = std::min(firstKf[std::max(a, b)], std::min(a, b)); }
    if (a >= 0) firstShared = std::min(firstShared, a);
    if (b >= 0) firstShared = std::min(firstShared, b);
  }
  EnvelopePlan Pl;
  {
    std::vector<int> eI(n), eJ(n);
    std::vector<uint8_t> nofix(n, 0);
    for (int a = 0; a < nSys; ++a) {
      const int k = sysKF[a], first = off[sysKF[firstKf[a]]] / 3;
      for (int r = off[k] / 3; r < (off[k] + wid[k]) / 3; ++r) { eI[r] = first; eJ[r] = r; }
    }
    if (bInit) for (int r = rbB; r < n; ++r) { eI[r] = firstShared < nSys ? off[sysKF[firstShared]] / 3 : rbB; eJ[r] = r; }
    const EnvelopeFit fit = plan_envelope(n, nofix.data(), n, eI.data(), eJ.data(), FIBA_MAX_BLOCKS, Pl);
    MORB_REQUIRE(fit == EnvelopeFit::Ok, MORB_ERR_CAPACITY, "the envelope of the reduced system exceeds what the handle may grow to");
  }
  const int nBlocks = Pl.nBlocks;
  if (pbStopFlag && *(const volatile uint8_t*)pbStopFlag) return nothing();   // (:689-690; behind the refusals: a refused call is refused whatever the flag says)
  auto blockOf = [&](int row, int col) { return Pl.rowOff[row] + (col - Pl.rowFirst[row]); };
  std::vector<int> pairOff(nPairs), pairSys(nPairs), blkDiag(nBlocks, -1), blkVis(nBlocks, -1), rowVis(n, -1);
  for (int p = 0; p < nPairs; ++p) { pairOff[p] = off[pairKF[p]]; pairSys[p] = sysIdx[pairKF[p]]; }
  for (int r = 0; r < n; ++r) blkDiag[Pl.rowOff[r + 1] - 1] = r;
  for (int a = 0; a < nSys; ++a) {
    const int r = off[sysKF[a]] / 3;
    blkVis[blockOf(r, r)] = a * 4; blkVis[blockOf(r + 1, r)] = a * 4 + 1; blkVis[blockOf(r + 1, r + 1)] = a * 4 + 2;
    rowVis[r] = a * 2; rowVis[r + 1] = a * 2 + 1;
  }
  std::vector<int> kfStart, kfEdges, kfPairStart, kfPairs;
  {
    std::vector<int> eSys(nE);
    for (int e = 0; e < nE; ++e) eSys[e] = sysIdx[eKF[e]] >= 0 ? sysIdx[eKF[e]] : nSys;
    std::vector<int> want(nSys + 1, 0);
    want[nSys] = -1;
    csr_by_key(eSys.data(), nE, nSys + 1, kfStart, kfEdges, want.data());
    kfStart.pop_back();
  }
  csr_by_key(pairSys.data(), nPairs, nSys, kfPairStart, kfPairs);
  std::vector<int> chunkKey, chunkStart, chunkEnd, blkChunkStart;
  std::vector<int2> ct(nCt);
  {
    std::vector<int> key(nCt), pos, ctStart;
    std::vector<int2> item(nCt);
    size_t q = 0;
    for (int m = 0; m < nMP; ++m)
      for (int p1 = mpPairStart[m]; p1 < mpPairStart[m + 1]; ++p1)
        for (int p2 = mpPairStart[m]; p2 <= p1; ++p2)   // (pairs ascend by keyframe within a point: p1's rows are not above p2's)
          for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) {
              const int row = pairOff[p1] / 3 + i, col = pairOff[p2] / 3 + j;
              if (row < col) continue;
              key[q] = blockOf(row, col);
              item[q].x = p1 * 2 + i; item[q].y = p2 * 2 + j;
              ++q;
            }
    csr_by_key(key.data(), (int)nCt, nBlocks, ctStart, pos);
    for (size_t k = 0; k < nCt; ++k) ct[k] = item[pos[k]];
    std::vector<int> all(nBlocks, 0);
    chunks_of(ctStart, all.data(), FIBA_CHUNK, chunkKey, chunkStart, chunkEnd, &blkChunkStart);
  }
  const int nChunks = (int)chunkKey.size();
  MORB_REQUIRE(nI < (1 << 23), MORB_ERR_CAPACITY, "more links than a contribution item indexes");   // (link * 256 + ... in an int)
  // where a link's record lands: its ten blocks of three columns on the system's block rows (-1: a fixed keyframe's, or none)
  std::vector<int> blkLinkStart, blkLinks, rowLinkStart, rowLinks;
  {
    std::vector<int> bKey, bItem, rKey, rItem, pos;
    for (int i = 0; i < nI; ++i) {
      int rows[10];
      const int o1 = off[iKF1[i]], o2 = off[iKF2[i]];
      for (int q = 0; q < 5; ++q) rows[q] = o1 >= 0 ? o1 / 3 + q : -1;
      for (int q = 0; q < 5; ++q) rows[5 + q] = o2 >= 0 ? o2 / 3 + q : -1;
      if (bInit) { rows[3] = rbB; rows[4] = rbB + 1; rows[8] = rows[9] = -1; }
      for (int qa = 0; qa < 10; ++qa) {
        if (rows[qa] < 0) continue;
        rKey.push_back(rows[qa]); rItem.push_back(i * 16 + qa);
        for (int qb = 0; qb < 10; ++qb) {
          if (rows[qb] < 0 || rows[qb] > rows[qa]) continue;
          bKey.push_back(blockOf(rows[qa], rows[qb])); bItem.push_back(i * 256 + qa * 16 + qb);
        }
      }
    }
    csr_by_key(bKey.data(), (int)bKey.size(), nBlocks, blkLinkStart, pos);
    blkLinks.resize(pos.size());
    for (size_t k = 0; k < pos.size(); ++k) blkLinks[k] = bItem[pos[k]];
    csr_by_key(rKey.data(), (int)rKey.size(), n, rowLinkStart, pos);
    rowLinks.resize(pos.size());
    for (size_t k = 0; k < pos.size(); ++k) rowLinks[k] = rItem[pos[k]];
  }
  const int nI1 = std::max(nI, 1);
  std::vector<double> InfoI((size_t)nI1 * 81, 0.0), InfoG((size_t)nI1 * 9, 0.0), InfoA((size_t)nI1 * 9, 0.0);
  for (int i = 0; i < nI; ++i) {
    fiba_inertial_information(iPre[i].C, &InfoI[(size_t)i * 81]);
    double Cg[9], Ca[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { Cg[r * 3 + c] = iPre[i].C[(9 + r) * 15 + 9 + c]; Ca[r * 3 + c] = iPre[i].C[(12 + r) * 15 + 12 + c]; }
    if (!fiba_invert(Cg, 3, &InfoG[(size_t)i * 9])) std::fill_n(&InfoG[(size_t)i * 9], 9, 0.0);
    if (!fiba_invert(Ca, 3, &InfoA[(size_t)i * 9])) std::fill_n(&InfoA[(size_t)i * 9], 9, 0.0);
  }
  const float zeros6[6] = {0, 0, 0, 0, 0, 0};

  MORB_ENTER(st, o, nullptr);
  FibaDev D;
  memset(&D, 0, sizeof D);
  D.nKF = nKF; D.nMP = nMP; D.nE = nE; D.nI = nI; D.nSys = nSys; D.n = n; D.P = P; D.nBlocks = nBlocks; D.nPairs = nPairs; D.nChunks = nChunks;
  D.maxIts = its; D.bInit = bInit; D.nChi = nE + nI + (bInit ? 2 : 0); D.rbB = bInit ? rbB : n;
  D.priorG = (double)priorG; D.priorA = (double)priorA;
  make_geom(Tbc12, cam5 ? cam5[0] : 0.f, cam5 ? cam5[1] : 0.f, cam5 ? cam5[2] : 0.f, cam5 ? cam5[3] : 0.f, cam5 ? cam5[4] : 0.f, rig28, D.g);
  ArenaCarver A;
  auto carve = [&]() {
    auto ints = [&](const std::vector<int>& v) { return (const int*)A.take(v.data(), sizeof(int) * v.size()); };
    auto dbls = [&](size_t cnt) { return (double*)A.take(nullptr, sizeof(double) * cnt); };
    D.eKF = (const int*)A.take(eKF, sizeof(int) * nE); D.eMP = (const int*)A.take(eMP, sizeof(int) * nE);
    D.eObs = (const float*)A.take(eObs, sizeof(float) * 3 * nE); D.eInfo = (const float*)A.take(eInvSigma2, sizeof(float) * nE);
    D.eRight = eRight ? (const uint8_t*)A.take(eRight, nE) : nullptr;
    D.off = ints(off); D.wid = ints(wid); D.sysIdx = ints(sysIdx); D.kfStart = ints(kfStart); D.kfEdges = ints(kfEdges);
    D.mpStart = ints(mpStart); D.mpEdges = ints(mpEdges); D.pairStart = ints(pairStart); D.pairEdges = ints(pairEdges);
    D.pairOff = ints(pairOff); D.pairMp = ints(pairMp); D.mpPairStart = ints(mpPairStart); D.kfPairStart = ints(kfPairStart); D.kfPairs = ints(kfPairs);
    D.rowFirst = ints(Pl.rowFirst); D.rowOff = ints(Pl.rowOff); D.colStart = ints(Pl.colStart); D.colRows = ints(Pl.colRows);
    D.blkDiag = ints(blkDiag); D.blkVis = ints(blkVis); D.rowVis = ints(rowVis);
    D.blkLinkStart = ints(blkLinkStart); D.blkLinks = ints(blkLinks); D.rowLinkStart = ints(rowLinkStart); D.rowLinks = ints(rowLinks);
    D.chunkStart = ints(chunkStart); D.chunkEnd = ints(chunkEnd); D.blkChunkStart = ints(blkChunkStart);
    D.ct = (const int2*)A.take(ct.data(), sizeof(int2) * nCt);
    D.iKF1 = (const int*)A.take(nI ? iKF1 : (const int*)zeros6, sizeof(int) * nI1); D.iKF2 = (const int*)A.take(nI ? iKF2 : (const int*)zeros6, sizeof(int) * nI1);
    D.iPre = (const morb_imu_preintegrated*)A.take(nI ? (const void*)iPre : (const void*)zeros6, nI ? sizeof(morb_imu_preintegrated) * nI : sizeof zeros6);
    D.InfoI = (const double*)A.take(InfoI.data(), sizeof(double) * InfoI.size()); D.InfoG = (const double*)A.take(InfoG.data(), sizeof(double) * InfoG.size());
    D.InfoA = (const double*)A.take(InfoA.data(), sizeof(double) * InfoA.size());
    D.kfIn = (const float*)A.take(kfState21, sizeof(float) * 21 * nKF); D.mpIn = (const float*)A.take(mpPos, sizeof(float) * 3 * nMP);
    D.biasIn = (const float*)A.take(bInit ? bias6 : zeros6, sizeof(float) * 6);
    D.S = dbls((size_t)33 * nKF); D.ST = dbls((size_t)33 * nKF); D.sb = dbls(6); D.sbT = dbls(6);
    D.pt = dbls((size_t)3 * nMP); D.ptT = dbls((size_t)3 * nMP);
    D.E = dbls((size_t)FIBA_EDGE * nE); D.LR = dbls((size_t)FIBA_LREC * nI1);
    D.Hpp = dbls((size_t)36 * nSys); D.bp = dbls((size_t)6 * nSys);
    D.Hll = dbls((size_t)9 * nMP); D.bl = dbls((size_t)3 * nMP); D.Dinv = dbls((size_t)9 * nMP); D.xl = dbls((size_t)3 * nMP);
    D.Hpl = dbls((size_t)18 * std::max(nPairs, 1)); D.HplD = dbls((size_t)18 * std::max(nPairs, 1)); D.hg = dbls((size_t)6 * std::max(nPairs, 1));
    D.part = dbls((size_t)9 * std::max(nChunks, 1));
    D.H = dbls((size_t)9 * nBlocks); D.L = dbls((size_t)9 * nBlocks);
    D.b0 = dbls(P); D.b = dbls(P); D.y = dbls(P); D.x = dbls(P); D.d = dbls(P);
    D.chiE = dbls(D.nChi);
    D.lm = (LmControl*)A.take(nullptr, sizeof(LmControl)); D.chi2 = dbls(2);
    D.lmi = (int*)A.take(nullptr, sizeof(int) * 8);
  };
  carve();   // (dry: sizes)
  char *arena = nullptr, *stage = nullptr;
  { const int rc = grow(o->fullInertialBA, A.uploadBytes() + A.deviceBytes(), &arena); if (rc != MORB_OK) return rc; }
  { const int rc = grow(o->stage, A.uploadBytes(), &stage); if (rc != MORB_OK) return rc; }
  A.bind(arena, stage);
  carve();
  if (!A.ok()) { set_error("the two carve passes of FullInertialBA differ"); return MORB_ERR_HIP; }
  int *hostw = nullptr, *hostwDev = nullptr;
  MORB_REQUIRE(morb_optimizer_lm_words(o, &hostw, &hostwDev) == MORB_OK, MORB_ERR_HIP, "cannot map the LM state words");
  D.lmHost = hostwDev;
  const volatile uint8_t* userStop = pbStopFlag;
  auto forwardStop = [&]() { if (userStop && *userStop) __atomic_store_n(hostw + 2, 1, __ATOMIC_RELEASE); };   // optimizer.setForceStopFlag(pbStopFlag) (:388)
  reset_lm_words(hostw, 2, hostw + 2);
  forwardStop();
  MORB_HIP_CHECK(hipMemcpyAsync(arena, stage, A.uploadBytes(), hipMemcpyHostToDevice, st));   // the one upload
  // the workspace is reused from call to call: what the first kernels expect to find zero is cleared
  MORB_HIP_CHECK(hipMemsetAsync(D.lmi, 0, sizeof(int) * 8, st));
  MORB_HIP_CHECK(hipMemsetAsync(D.lm, 0, sizeof(LmControl), st));
  MORB_HIP_CHECK(hipMemsetAsync(D.x, 0, sizeof(double) * P, st));        // the step before the first solve
  MORB_HIP_CHECK(hipMemsetAsync(D.xl, 0, sizeof(double) * 3 * nMP, st));

  auto blocks = [](size_t items) { return dim3((unsigned)((items + FIBA_NT - 1) / FIBA_NT)); };
  const dim3 chiBlocks = blocks((size_t)D.nChi), edgeBlocks = blocks((size_t)nE);
  const size_t asmItems = (size_t)nSys * 42 + (size_t)nMP * 12 + (size_t)nPairs * 18;
  const size_t finItems = (size_t)nBlocks * 9 + (size_t)P;
  hipLaunchKernelGGL(k_fiba_setup, blocks((size_t)std::max(std::max(nKF, 3 * nMP), 6)), dim3(FIBA_NT), 0, st, D);
  hipLaunchKernelGGL(k_fiba_errors, chiBlocks, dim3(FIBA_NT), 0, st, D, 0);   // computeActiveErrors
  hipLaunchKernelGGL(k_fiba_decide, dim3(1), dim3(FIBA_NT), 0, st, D, 1);
  MORB_HIP_CHECK(hipGetLastError());
  // a slot is one trial: at most `its` iterations of 10 trials
  const int q = lm_slot_queue(10 * its, hostw + 0, hostw + 1, [&](int) {
    if (rig28) hipLaunchKernelGGL(k_fiba_linearize<true>, edgeBlocks, dim3(FIBA_NT), 0, st, D);   // (the first three run only behind an accepted trial)
    else hipLaunchKernelGGL(k_fiba_linearize<false>, edgeBlocks, dim3(FIBA_NT), 0, st, D);
    if (nI) hipLaunchKernelGGL(k_fiba_links, dim3(nI), dim3(64), 0, st, D);
    hipLaunchKernelGGL(k_fiba_assemble, blocks(asmItems), dim3(FIBA_NT), 0, st, D);
    hipLaunchKernelGGL(k_fiba_dinv, blocks((size_t)nMP + nPairs), dim3(FIBA_NT), 0, st, D);
    if (nChunks) hipLaunchKernelGGL(k_fiba_schur, blocks((size_t)nChunks * 9), dim3(FIBA_NT), 0, st, D);
    hipLaunchKernelGGL(k_fiba_finish, blocks(finItems), dim3(FIBA_NT), 0, st, D);
    hipLaunchKernelGGL(k_fiba_factor, dim3(1), dim3(FIBA_NT), 0, st, D);
    hipLaunchKernelGGL(k_fiba_backsub, dim3(1), dim3(FIBA_NT), 0, st, D);
    hipLaunchKernelGGL(k_fiba_points, blocks((size_t)nMP), dim3(FIBA_NT), 0, st, D);
    hipLaunchKernelGGL(k_fiba_errors, chiBlocks, dim3(FIBA_NT), 0, st, D, 1);
    hipLaunchKernelGGL(k_fiba_decide, dim3(1), dim3(FIBA_NT), 0, st, D, 0);
    if (hipGetLastError() != hipSuccess) { set_error("FullInertialBA: a trial's launch failed"); return (int)MORB_ERR_HIP; }
    return (int)MORB_OK;
  }, [&]() { return stream_look(st, "FullInertialBA"); }, forwardStop);
  if (q < 0) return MORB_ERR_HIP;
  int hi[8];
  double c2[2], sb[6];
  std::vector<double> S((size_t)33 * nKF), pt((size_t)3 * nMP);
  MORB_HIP_CHECK(hipMemcpyAsync(hi, D.lmi, sizeof hi, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipMemcpyAsync(c2, D.chi2, sizeof c2, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipMemcpyAsync(sb, D.sb, sizeof sb, hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipMemcpyAsync(S.data(), D.S, sizeof(double) * S.size(), hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipMemcpyAsync(pt.data(), D.pt, sizeof(double) * pt.size(), hipMemcpyDeviceToHost, st));
  MORB_HIP_CHECK(hipStreamSynchronize(st));   // (also drains a queue that ran out of slots before the words are reset again)
  // (:696-757) the keyframes of the system — kind 3 in the pose only; with bInit every kind-0 keyframe gets the shared biases (:719-738) —
  // and the points that carry an edge; everything else keeps its bytes
  for (int v = 0; v < nKF; ++v) {
    if (off[v] < 0) continue;
    float* s = kfState21 + 21 * (size_t)v;
    for (int k = 0; k < (wid[v] == 6 ? 12 : 15); ++k) s[k] = (float)S[(size_t)33 * v + k];
    if (wid[v] == 15) for (int k = 15; k < 21; ++k) s[k] = (float)S[(size_t)33 * v + k];
    if (wid[v] == 9) for (int k = 0; k < 6; ++k) s[15 + k] = (float)sb[k];
  }
  if (bInit) for (int k = 0; k < 6; ++k) bias6[k] = (float)sb[k];
  for (int m = 0; m < nMP; ++m) if (mpStart[m + 1] > mpStart[m]) for (int k = 0; k < 3; ++k) mpPos[3 * m + k] = (float)pt[(size_t)3 * m + k];
  stats4[0] = hi[LMW_ITS]; stats4[1] = hi[LMW_TRIALS]; stats4[2] = P; stats4[3] = nBlocks;
  chi2[0] = c2[0]; chi2[1] = c2[1];
  return MORB_OK;
}

}  // namespace

extern "C" int morb_full_inertial_ba(morb_optimizer* o, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos, int nE,
                                     const int* eKF, const int* eMP, const float* eObs, const float* eInvSigma2, int nI, const int* iKF1,
                                     const int* iKF2, const morb_imu_preintegrated* iPre, float fx, float fy, float cx, float cy, float bf,
                                     const float* Tbc12, int its, int bInit, float priorG, float priorA, float* bias6,
                                     const uint8_t* pbStopFlag, int* stats4, double* chi2) {
  const float cam5[5] = {fx, fy, cx, cy, bf};
  return fiba_run(o, nKF, kfState21, kfKind, nMP, mpPos, nE, eKF, eMP, eObs, nullptr, eInvSigma2, nI, iKF1, iKF2, iPre, cam5, nullptr, Tbc12, its,
                  bInit, priorG, priorA, bias6, pbStopFlag, stats4, chi2);
}

extern "C" int morb_full_inertial_ba_fisheye(morb_optimizer* o, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos, int nE,
                                             const int* eKF, const int* eMP, const float* eObs, const uint8_t* eRight, const float* eInvSigma2,
                                             int nI, const int* iKF1, const int* iKF2, const morb_imu_preintegrated* iPre, const float* rig28,
                                             const float* Tbc12, int its, int bInit, float priorG, float priorA, float* bias6,
                                             const uint8_t* pbStopFlag, int* stats4, double* chi2) {
  MORB_REQUIRE(eRight && rig28, MORB_ERR_INVALID, "NULL argument");
  return fiba_run(o, nKF, kfState21, kfKind, nMP, mpPos, nE, eKF, eMP, eObs, eRight, eInvSigma2, nI, iKF1, iKF2, iPre, nullptr, rig28, Tbc12, its,
                  bInit, priorG, priorA, bias6, pbStopFlag, stats4, chi2);
}
