// Visual-inertial tracking slice of SURVEY §8(f) row N1 for MI355X (gfx950):
//   IMU::Preintegrated::IntegrateNewMeasurement        (reference src/ImuTypes.cc:191-247)      -> k_imu_preintegrate, one thread per
//                                                        measurement sequence (the recursion is sequential; frames are independent)
//   Optimizer::PoseInertialOptimizationLastKeyFrame    (reference src/Optimizer.cc:4391-4757)   -> k_pose_inertial, one workgroup per
//                                                        frame, the whole 4 x 10 Gauss-Newton schedule in ONE launch
// g2o semantics kept: Gauss-Newton (computeActiveErrors, buildSystem, dense LDL^T, update; optimization_algorithm_gauss_newton.cpp:
// 51-96), Huber weights through rho' (base_unary_edge.hpp:43-72), inlier edges keep the error of the state BEFORE the last update,
// outlier edges are re-evaluated at the final state (Optimizer.cc:4628-4640), float chi2 comparisons.
// State layout (floats at the boundary, FP64 inside): Rwb (9, row-major), twb (3), velocity (3), gyro bias (3), acc bias (3).
// The visual edges (hundreds per frame) are spread over the workgroup and reduced with wave shuffles; the 9-D inertial edge, the
// two random-walk edges and the 15 x 15 solve are wave-uniform arithmetic every thread repeats in registers (no broadcast of
// the state is needed: all threads apply the same update).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "common.h"
#include "internal_abi.h"
#include "libm_f32.h"
#include "wave.h"
#include "inertial_device.h"

using namespace morb;

#define WAVE_SYNC()                                        \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); \
    __builtin_amdgcn_wave_barrier();                       \
  } while (0)

namespace {

// One wave per measurement sequence (the recursion over the samples is sequential, sequences are independent).  Lane 0 carries the
// 3 x 3 state (rotation, velocity, position, bias Jacobians) and writes the sample's A (9 x 9) and B (9 x 6) to LDS; the 64 lanes
// then share the two dense 9 x 9 covariance products, each entry summed in the reference's order.
__global__ __launch_bounds__(64) void k_imu_preintegrate(int nseq, const int* __restrict__ start, const float* __restrict__ acc,
                                                         const float* __restrict__ gyro, const float* __restrict__ dts,
                                                         const float* __restrict__ bias, morb_imu_preintegrated calib,
                                                         morb_imu_preintegrated* __restrict__ out) {
  __shared__ float sA[81], sB[54], sC[81], sAC[81];
  const int s = blockIdx.x, lane = threadIdx.x;
  if (s >= nseq) return;
  float dR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, dV[3] = {0, 0, 0}, dP[3] = {0, 0, 0};
  float JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], avgA[3] = {0, 0, 0}, avgW[3] = {0, 0, 0}, b[6], dT = 0.f, walk[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 9; ++k) { JRg[k] = 0; JVg[k] = 0; JVa[k] = 0; JPg[k] = 0; JPa[k] = 0; }
  for (int k = 0; k < 6; ++k) b[k] = bias[6 * s + k];
  for (int k = lane; k < 81; k += 64) sC[k] = 0.f;
  const int i0 = start[s], i1 = start[s + 1];
  for (int i = i0; i < i1; ++i) {
    const float dt = dts[i];
    if (lane == 0) {
      const float a[3] = {acc[3 * i] - b[0], acc[3 * i + 1] - b[1], acc[3 * i + 2] - b[2]};
      const float wv[3] = {gyro[3 * i] - b[3], gyro[3 * i + 1] - b[4], gyro[3 * i + 2] - b[5]};
      float Racc[3];
      mul3v(dR, a, Racc);
      for (int k = 0; k < 3; ++k) {
        avgA[k] = (dT * avgA[k] + Racc[k] * dt) / (dT + dt);
        avgW[k] = (dT * avgW[k] + wv[k] * dt) / (dT + dt);
      }
      for (int k = 0; k < 3; ++k) {
        dP[k] = dP[k] + dV[k] * dt + 0.5f * Racc[k] * dt * dt;
        dV[k] = dV[k] + Racc[k] * dt;
      }
      // scalar factors where the C++ expressions apply them (:217-226): -dR * dt * Wacc = ((-dR) * dt) * Wacc,
      // 0.5f * dR * dt * dt * Wacc * JRg = ((((0.5f * dR) * dt) * dt) * Wacc) * JRg
      float Wacc[9], Rdt[9], Rhdt2[9], RdtW[9], Rhdt2W[9], RdtWJ[9], Rhdt2WJ[9];
      hatf(a, Wacc);
      for (int k = 0; k < 9; ++k) { Rdt[k] = dR[k] * dt; Rhdt2[k] = 0.5f * dR[k] * dt * dt; }
      mul33(Rdt, Wacc, RdtW);
      mul33(Rhdt2, Wacc, Rhdt2W);
      mul33(RdtW, JRg, RdtWJ);
      mul33(Rhdt2W, JRg, Rhdt2WJ);
      // A = [dRi^T 0 0; -dR dt Wacc, I, 0; -dR dt^2/2 Wacc, I dt, I],  B = [rightJ dt, 0; 0, dR dt; 0, dR dt^2/2]
      for (int k = 0; k < 81; ++k) sA[k] = 0.f;
      for (int k = 0; k < 54; ++k) sB[k] = 0.f;
      for (int k = 0; k < 9; ++k) sA[k * 9 + k] = 1.f;
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
          sA[(3 + r) * 9 + c] = -RdtW[r * 3 + c]; sA[(6 + r) * 9 + c] = -Rhdt2W[r * 3 + c];
          sB[(3 + r) * 6 + 3 + c] = Rdt[r * 3 + c]; sB[(6 + r) * 6 + 3 + c] = Rhdt2[r * 3 + c];
        }
      for (int k = 0; k < 3; ++k) sA[(6 + k) * 9 + 3 + k] = dt;
      for (int k = 0; k < 9; ++k) {
        JPa[k] = JPa[k] + JVa[k] * dt - Rhdt2[k];
        JPg[k] = JPg[k] + JVg[k] * dt - Rhdt2WJ[k];
        JVa[k] = JVa[k] - Rdt[k];
        JVg[k] = JVg[k] - RdtWJ[k];
      }
      // IntegratedRotation (ImuTypes.cc:84-107)
      float dRi[9], rJ[9];
      {
        const float x = wv[0] * dt, y = wv[1] * dt, z = wv[2] * dt;
        const float d2 = x * x + y * y + z * z, d = sqrtf(d2);
        const float v[3] = {x, y, z};
        float W[9], WW[9];
        hatf(v, W);
        mul33(W, W, WW);
        if (d < 1e-4f) {
          for (int k = 0; k < 9; ++k) { dRi[k] = ((k & 3) == 0 ? 1.f : 0.f) + W[k]; rJ[k] = (k & 3) == 0 ? 1.f : 0.f; }
        } else {
          const float sn = morbm::sinf_glibc(d), cs = morbm::cosf_glibc(d);
          for (int k = 0; k < 9; ++k) {
            const float I = (k & 3) == 0 ? 1.f : 0.f;
            dRi[k] = I + W[k] * sn / d + WW[k] * (1.0f - cs) / d2;
            rJ[k] = I - W[k] * (1.0f - cs) / d2 + WW[k] * (d - sn) / (d2 * d);
          }
        }
      }
      mul33(dR, dRi, dR);
      normalize_rotation_f(dR);
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) { sA[r * 9 + c] = dRi[c * 3 + r]; sB[r * 6 + c] = rJ[r * 3 + c] * dt; }
      float dRiT[9], t9[9];
      for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) dRiT[r * 3 + c] = dRi[c * 3 + r];
      mul33(dRiT, JRg, t9);
      for (int k = 0; k < 9; ++k) JRg[k] = t9[k] - rJ[k] * dt;
      dT += dt;
      for (int k = 0; k < 6; ++k) walk[k] += calib.ngaWalk[k];
    }
    WAVE_SYNC();
    // C(0:9,0:9) = A C A^T + B Nga B^T, dense like the reference (zeros included, k ascending)
    for (int idx = lane; idx < 81; idx += 64) {
      const int r = idx / 9, c = idx - r * 9;
      float sum = 0;
      for (int k = 0; k < 9; ++k) sum += sA[r * 9 + k] * sC[k * 9 + c];
      sAC[idx] = sum;
    }
    WAVE_SYNC();
    float nv[2] = {0.f, 0.f};
    for (int q = 0, idx = lane; idx < 81; idx += 64, ++q) {
      const int r = idx / 9, c = idx - r * 9;
      float sum = 0;
      for (int k = 0; k < 9; ++k) sum += sAC[r * 9 + k] * sA[c * 9 + k];
      float t = 0;
      for (int k = 0; k < 6; ++k) t += sB[r * 6 + k] * calib.nga[k] * sB[c * 6 + k];
      nv[q] = sum + t;
    }
    WAVE_SYNC();
    for (int q = 0, idx = lane; idx < 81; idx += 64, ++q) sC[idx] = nv[q];
    WAVE_SYNC();
  }
  morb_imu_preintegrated* o = out + s;
  for (int k = lane; k < 225; k += 64) {
    const int r = k / 15, c = k - r * 15;
    o->C[k] = (r < 9 && c < 9) ? sC[r * 9 + c] : 0.f;
  }
  WAVE_SYNC();
  if (lane == 0) {
    o->dT = dT;
    for (int k = 0; k < 9; ++k) { o->dR[k] = dR[k]; o->JRg[k] = JRg[k]; o->JVg[k] = JVg[k]; o->JVa[k] = JVa[k]; o->JPg[k] = JPg[k]; o->JPa[k] = JPa[k]; }
    for (int k = 0; k < 3; ++k) { o->dV[k] = dV[k]; o->dP[k] = dP[k]; o->avgA[k] = avgA[k]; o->avgW[k] = avgW[k]; }
    for (int k = 0; k < 6; ++k) { o->b[k] = b[k]; o->nga[k] = calib.nga[k]; o->ngaWalk[k] = calib.ngaWalk[k]; o->C[(9 + k) * 15 + 9 + k] = walk[k]; }
  }
}

// ---- per-frame workspace in LDS ------------------------------------------------------------------------------------------------
// The visual edges are spread over the 256 threads; the few dense edges (inertial 9 x 24, prior 15 x 15) are written into LDS by
// one thread and multiplied out by all of them; the dense solve runs in wave 0 on the LDS matrix.
struct InertialWork {
  double H[30 * 30], b[30], x[32];
  double J[9 * 24], OJ[9 * 24], e[9], Oe[9];          // inertial edge (columns in edge order P1 V1 G1 A1 P2 V2)
  double Jp[15 * 15], OJp[15 * 15], ep[15], Oep[15];  // prior edge (last-frame variant); scratch for the one-off 9 x 9 / 15 x 15 work
  double InfoI[81], InfoG[9], InfoA[9];
  double pH[225];                                     // prior information
  double red[4][28];
  double delta[18];                                   // dR dV dP dbg of the inertial edge while state 1 is fixed
  double wPrior;
  int cnt[4][2];
  int flag;
};

// LinearSolverDense (linear_solver_dense.h:104-112): LDL^T solve, solution only when every pivot is positive.  ONE wave; lane r
// keeps row r of the matrix in registers, column entries of other rows arrive through v_readlane (the loops are fully
// unrolled, so every register index and every source lane is a compile-time constant): no LDS round trip and no barrier in
// the factorisation or the forward substitution.  The backward substitution needs L transposed: the rows go to LDS once.
template <int N>
__device__ bool wave_ldlt_solve(const double* H, int ld, const double* rhs, double* x, double* Lscr, int lane) {
  const int row = lane < N ? lane : N - 1;   // lanes >= N replicate the last row; their results are not used
  double a[N];
#pragma unroll
  for (int c = 0; c < N; ++c) a[c] = H[row * ld + c];
  double y = rhs[row], diag = 1.0;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double d = morbwave::readlane_f64(a[j], j);
    ok = ok && (d > 0);
    if (row == j) diag = d;
    const double l = a[j] / d;
#pragma unroll
    for (int c = j + 1; c < N; ++c) a[c] -= l * morbwave::readlane_f64(a[j], c);   // A[r][c] -= A[r][j] A[c][j] / d
    a[j] = l;
  }
  if (!ok) return false;   // wave-uniform
#pragma unroll
  for (int j = 0; j < N - 1; ++j) {   // L y = b
    const double yj = morbwave::readlane_f64(y, j);
    if (row > j) y -= a[j] * yj;
  }
  y /= diag;
#pragma unroll
  for (int c = 0; c < N; ++c) Lscr[row * N + c] = a[c];
  WAVE_SYNC();
#pragma unroll
  for (int j = N - 1; j > 0; --j) {   // L^T x = y
    const double xj = morbwave::readlane_f64(y, j);
    if (row < j) y -= Lscr[j * N + row] * xj;
  }
  if (lane < N) x[lane] = y;
  WAVE_SYNC();
  return true;
}

// EdgePriorPoseImu (G2oTypes.cc:739-766): error (15) and the 15 x 15 Jacobian in LDS.  prior = Rwb twb v bg ba (21 doubles).
__device__ void prior_edge(const double* prior, const VIState& S1, double* err, double* J) {
  double pRt[9], E[9], er[3], d[3], et[3];
  transpose33(prior, pRt);
  mul33(pRt, S1.Rwb, E);
  log_so3(E, er);
  for (int k = 0; k < 3; ++k) d[k] = S1.twb[k] - prior[9 + k];
  mul3v(pRt, d, et);
  for (int k = 0; k < 3; ++k) { err[k] = er[k]; err[3 + k] = et[k]; err[6 + k] = S1.v[k] - prior[12 + k]; err[9 + k] = S1.bg[k] - prior[15 + k]; err[12 + k] = S1.ba[k] - prior[18 + k]; }
  if (!J) return;   // J zeroed once by the caller
  double invJr[9];
  inv_right_jacobian_so3(er, invJr);
  put33(J, 15, 0, 0, invJr, 1.0);
  put33(J, 15, 3, 3, E, 1.0);
  for (int k = 6; k < 15; ++k) J[k * 15 + k] = 1.0;
}

// system column of an inertial-edge column: frame = [P 0..5, V 6..8, G 9..11, A 12..14], previous frame / keyframe = 15 + the same

// LASTFRAME = false: PoseInertialOptimizationLastKeyFrame (state 1 = the keyframe, fixed: 15 unknowns)
// LASTFRAME = true : PoseInertialOptimizationLastFrame   (state 1 = the previous frame, free, with its prior: 30 unknowns)
#ifdef MORB_INERTIAL_TIMING
__device__ unsigned long long g_inertialPhase[16];
#define IMARK(k) do { __syncthreads(); if (tid == 0 && blockIdx.x == 0) { const unsigned long long now_ = wall_clock64(); atomicAdd(&g_inertialPhase[k], now_ - t0_); t0_ = now_; } } while (0)
#else
#define IMARK(k)
#endif
// GEDGE: the edge list lives in global memory (frames whose cap * 32 bytes do not fit the LDS beside the kernel's static data: ~4900 features) instead of LDS
template <bool LASTFRAME, bool RIG, bool GEDGE>
__global__ __launch_bounds__(256) void k_pose_inertial(int cap, const int* __restrict__ count, const uint8_t* __restrict__ hasMP,
                                                       const float* __restrict__ obs, const float* __restrict__ invSigma2,
                                                       const float* __restrict__ Xw, const uint8_t* __restrict__ closeFlag,
                                                       CamGeom g, const float* __restrict__ state1,
                                                       const morb_imu_preintegrated* __restrict__ pre,
                                                       const morb_imu_preintegrated* __restrict__ preKF,
                                                       const double* __restrict__ prevPrior, const int* __restrict__ nLeft,
                                                       int bRecInit, float* __restrict__ stateIO, uint8_t* __restrict__ outlier,
                                                       int* __restrict__ nInliersOut, double* __restrict__ prior, float* __restrict__ gEdge) {
  __shared__ InertialWork Wk;
  // the round's ACTIVE visual edges (map point present, not an outlier of the round before), compacted in feature order: (u, v, uR | X | info | camera)
  // as eight floats per edge.  The ten Gauss-Newton iterations of a round read them from here: each of a thread's three to five edges used to start
  // with a dependent round trip to global memory for its flags and another for its data (~2 k cycles per edge beside ~2.6 k of arithmetic).
  extern __shared__ __align__(16) float sEdgeLds[];
  float* const sEdge = GEDGE ? gEdge + (size_t)blockIdx.x * cap * 8 : sEdgeLds;   // (a compile-time choice: each instantiation knows its address space)
  __shared__ VIState sS1;   // state 1 (keyframe / previous frame): only the dense-edge threads read it, one thread updates it
  constexpr int NV = LASTFRAME ? 30 : 15;
  // threads on the visual edges; wave 3 evaluates the inertial edge and (last-frame variant) wave 2 the prior edge meanwhile
  constexpr int NVIS = LASTFRAME ? 128 : 192, NVW = NVIS / 64;
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = count ? count[f] : cap;
  const size_t base = (size_t)f * cap;
  const double deltaMono = (double)(float)sqrt(5.991), deltaStereo = (double)(float)sqrt(7.815);
  const morb_imu_preintegrated& P = pre[f];
  const double* pr = LASTFRAME ? prevPrior + (size_t)246 * f : nullptr;
  const int nL = RIG ? nLeft[f] : n;   // fisheye rig: features >= nL are right-camera observations; every edge is monocular

  int nInit = 0;
  for (int i = tid; i < n; i += 256) if (hasMP[base + i]) { ++nInit; outlier[base + i] = 0; }
  nInit = (int)wave_sum((double)nInit);
  if (lane == 0) Wk.cnt[wv][0] = nInit;
  __syncthreads();
  nInit = Wk.cnt[0][0] + Wk.cnt[1][0] + Wk.cnt[2][0] + Wk.cnt[3][0];
  __syncthreads();

  if (tid == 0) {   // informations: EdgeInertial (G2oTypes.cc:484-491), EdgeGyroRW / EdgeAccRW (Optimizer.cc:4580-4594)
    double* C9 = Wk.J;        // scratch: 81 + 162 + 162 doubles fit in J | OJ | Jp | OJp
    for (int r = 0; r < 9; ++r) for (int c = 0; c < 9; ++c) C9[r * 9 + c] = (double)P.C[r * 15 + c];
    if (invert_n(C9, 9, Wk.InfoI, Wk.Jp)) {
      for (int r = 0; r < 9; ++r) for (int c = r + 1; c < 9; ++c) { const double s = (Wk.InfoI[r * 9 + c] + Wk.InfoI[c * 9 + r]) / 2; Wk.InfoI[r * 9 + c] = s; Wk.InfoI[c * 9 + r] = s; }
      clamp_eigenvalues(Wk.InfoI, 9, 1e-12, Wk.Jp, Wk.OJp);
    } else for (int k = 0; k < 81; ++k) Wk.InfoI[k] = 0;
    const morb_imu_preintegrated& PK = LASTFRAME ? preKF[f] : P;
    double Cg[9], Ca[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { Cg[r * 3 + c] = PK.C[(9 + r) * 15 + 9 + c]; Ca[r * 3 + c] = PK.C[(12 + r) * 15 + 12 + c]; }
    if (!invert_n(Cg, 3, Wk.InfoG, Wk.Jp)) for (int k = 0; k < 9; ++k) Wk.InfoG[k] = 0;
    if (!invert_n(Ca, 3, Wk.InfoA, Wk.Jp)) for (int k = 0; k < 9; ++k) Wk.InfoA[k] = 0;
  }
  if (LASTFRAME) for (int k = tid; k < 225; k += 256) Wk.pH[k] = pr[21 + k];
  __syncthreads();

#ifdef MORB_INERTIAL_TIMING
  unsigned long long t0_ = wall_clock64();
#endif
  IMARK(0);
  VIState S, Sprev;   // Sprev: only its camera poses are ever assigned / read
  load_state_t<RIG>(g, stateIO + 21 * f, S);
  if (tid == 0) load_state_t<RIG>(g, state1 + 21 * f, sS1);
  const VIState& S1 = sS1;
  auto keep_cameras = [&]() {
    for (int k = 0; k < 9; ++k) { Sprev.Rcw[k] = S.Rcw[k]; if (RIG) Sprev.Rcw1[k] = S.Rcw1[k]; }
    for (int k = 0; k < 3; ++k) { Sprev.tcw[k] = S.tcw[k]; if (RIG) Sprev.tcw1[k] = S.tcw1[k]; }
  };
  keep_cameras();
  __syncthreads();   // the setup above used J / Jp as scratch; sS1 is visible
  for (int k = tid; k < 216; k += 256) Wk.J[k] = 0;
  for (int k = tid; k < 225; k += 256) Wk.Jp[k] = 0;
  if (!LASTFRAME && tid == 0) imu_delta(P, S1.bg, S1.ba, Wk.delta, Wk.delta + 9, Wk.delta + 12, Wk.delta + 15);
  __syncthreads();
  const double* delta = LASTFRAME ? nullptr : Wk.delta;
  auto redsum = [&](int q) { double s = 0; for (int w = 0; w < NVW; ++w) s += Wk.red[w][q]; return s; };
  bool robust = true;
  int nBad = 0, nInl = 0;
  for (int k = tid; k < 32; k += 256) Wk.x[k] = 0;
  const float chi2MonoKF[4] = {12.f, 7.5f, 5.991f, 5.991f}, chi2MonoF[4] = {5.991f, 5.991f, 5.991f, 5.991f};
  const float chi2Stereo[4] = {15.6f, 9.8f, 7.815f, 7.815f};

  for (int it = 0; it < 4; ++it) {
    bool ok = true;
    int nAct = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
      const int i = c0 + tid;
      const bool a = i < n && hasMP[base + i] && !outlier[base + i];
      const unsigned long long m = __ballot(a);
      if (lane == 0) Wk.cnt[wv][0] = __popcll(m);
      __syncthreads();
      int off = nAct, totc = 0;
      for (int w = 0; w < 4; ++w) { const int c = Wk.cnt[w][0]; if (w < wv) off += c; totc += c; }
      if (a) {
        float* r = sEdge + 8 * (size_t)(off + __popcll(m & ((1ull << lane) - 1ull)));
        r[0] = obs[(base + i) * 3]; r[1] = obs[(base + i) * 3 + 1]; r[2] = obs[(base + i) * 3 + 2];
        r[3] = Xw[(base + i) * 3]; r[4] = Xw[(base + i) * 3 + 1]; r[5] = Xw[(base + i) * 3 + 2];
        r[6] = invSigma2[base + i]; r[7] = i >= nL ? 1.0f : 0.0f;
      }
      nAct += totc;
      __syncthreads();
    }
    for (int iter = 0; iter < 10 && ok; ++iter) {
      IMARK(1);
      keep_cameras();   // the state the active edges' errors belong to
      // ---- visual edges -> 6 x 6 block and right-hand side of the frame's pose
      if (tid < NVIS) {
        double acc[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) acc[k] = 0;
        for (int e = tid; e < nAct; e += NVIS) {
          const float* o = sEdge + 8 * (size_t)e;
          const bool st = !RIG && !(o[2] < 0);
          const int cam = o[7] != 0.0f ? 1 : 0;
          const double X[3] = {(double)o[3], (double)o[4], (double)o[5]};
          const double info = (double)o[6];
          double err[3], Xc[3], J[18];
          const double c = vis_error_t<RIG>(g, S, X, o, st, info, err, Xc, cam);
          const double w = robust ? huber_w(st ? deltaStereo : deltaMono, c) : 1.0;
          vis_jacobian_t<RIG>(g, Xc, st, J, cam);   // a mono edge has a zero third row and err[2] = 0: one fully unrolled 3-row form (registers only)
          int q = 0;
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            double bb = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) bb += J[k * 6 + r] * (info * err[k]);
            acc[21 + r] -= w * bb;
#pragma unroll
            for (int cc = r; cc < 6; ++cc) {
              double h = 0;
#pragma unroll
              for (int k = 0; k < 3; ++k) h += J[k * 6 + r] * (w * info) * J[k * 6 + cc];
              acc[q++] += h;
            }
          }
        }
#pragma unroll
        for (int k = 0; k < 27; ++k) acc[k] = wave_sum(acc[k]);
        if (lane == 0) for (int k = 0; k < 27; ++k) Wk.red[wv][k] = acc[k];
      } else if (tid == 192) {
        inertial_edge(P, S1, S, delta, LASTFRAME, Wk.e, Wk.J);   // error + Jacobian to LDS
      } else if (LASTFRAME && tid == 128) {
        prior_edge(pr, S1, Wk.ep, Wk.Jp);
      }
      IMARK(2);
      __syncthreads();
      IMARK(3);
      // ---- Omega J, Omega e
      for (int k = tid; k < 9 * 24 + 9; k += 256) {
        if (k < 216) { const int r = k / 24, c = k - r * 24; double s = 0; for (int l = 0; l < 9; ++l) s += Wk.InfoI[r * 9 + l] * Wk.J[l * 24 + c]; Wk.OJ[k] = s; }
        else { const int r = k - 216; double s = 0; for (int l = 0; l < 9; ++l) s += Wk.InfoI[r * 9 + l] * Wk.e[l]; Wk.Oe[r] = s; }
      }
      if (LASTFRAME) {
        for (int k = tid; k < 225 + 15; k += 256) {
          if (k < 225) { const int r = k / 15, c = k - r * 15; double s = 0; for (int l = 0; l < 15; ++l) s += Wk.pH[r * 15 + l] * Wk.Jp[l * 15 + c]; Wk.OJp[k] = s; }
          else { const int r = k - 225; double s = 0; for (int l = 0; l < 15; ++l) s += Wk.pH[r * 15 + l] * Wk.ep[l]; Wk.Oep[r] = s; }
        }
      }
      __syncthreads();
      if (LASTFRAME && tid == 0) {   // Huber weight of the prior edge (delta 5, Optimizer.cc:4981-4984)
        double chi2 = 0;
        for (int k = 0; k < 15; ++k) chi2 += Wk.ep[k] * Wk.Oep[k];
        Wk.wPrior = huber_w(5.0, chi2);
      }
      if (LASTFRAME) __syncthreads();
      IMARK(4);
      // ---- H and b: every entry by one thread
      for (int k = tid; k < NV * NV + NV; k += 256) {
        if (k < NV * NV) {
          const int r = k / NV, c = k - r * NV;
          double h = 0;
          if (r < 6 && c < 6) {   // visual block (upper triangle was accumulated)
            const int a = r < c ? r : c, bq = r < c ? c : r;
            const int q = a * 6 - a * (a - 1) / 2 + (bq - a);
            h = redsum(q);
          }
          // inertial edge: system index -> edge column
          const int ea = r < 15 ? (r < 9 ? 15 + r : -1) : r - 15, ec = c < 15 ? (c < 9 ? 15 + c : -1) : c - 15;
          if (ea >= 0 && ec >= 0) { double s = 0; for (int l = 0; l < 9; ++l) s += Wk.J[l * 24 + ea] * Wk.OJ[l * 24 + ec]; h += s; }
          // random walks: e = bias2 - bias1 (G2oTypes.h:645-654)
          const int rb = r % 15, cb = c % 15;
          if (rb >= 9 && cb >= 9 && (rb < 12) == (cb < 12)) {
            const double* I3 = rb < 12 ? Wk.InfoG : Wk.InfoA;
            const double v = I3[(rb - (rb < 12 ? 9 : 12)) * 3 + (cb - (cb < 12 ? 9 : 12))];
            h += ((r < 15) == (c < 15)) ? v : -v;
          }
          if (LASTFRAME && r >= 15 && c >= 15) { double s = 0; for (int l = 0; l < 15; ++l) s += Wk.Jp[l * 15 + (r - 15)] * Wk.OJp[l * 15 + (c - 15)]; h += Wk.wPrior * s; }
          Wk.H[r * 30 + c] = h;
        } else {
          const int r = k - NV * NV;
          double s = 0;
          if (r < 6) s = redsum(21 + r);
          const int ea = r < 15 ? (r < 9 ? 15 + r : -1) : r - 15;
          if (ea >= 0) { double t = 0; for (int l = 0; l < 9; ++l) t += Wk.J[l * 24 + ea] * Wk.Oe[l]; s -= t; }
          const int rb = r % 15;
          if (rb >= 9) {
            const double* I3 = rb < 12 ? Wk.InfoG : Wk.InfoA;
            const double* b2 = rb < 12 ? S.bg : S.ba; const double* b1 = rb < 12 ? S1.bg : S1.ba;
            const int q = rb - (rb < 12 ? 9 : 12);
            double t = 0;
            for (int l = 0; l < 3; ++l) t += I3[q * 3 + l] * (b2[l] - b1[l]);
            s += r < 15 ? -t : t;   // J2 = I, J1 = -I
          }
          if (LASTFRAME && r >= 15) { double t = 0; for (int l = 0; l < 15; ++l) t += Wk.Jp[l * 15 + (r - 15)] * Wk.Oep[l]; s -= Wk.wPrior * t; }
          Wk.b[r] = s;
        }
      }
      __syncthreads();
      IMARK(5);
      if (wv == 0) {
        const bool good = wave_ldlt_solve<NV>(Wk.H, 30, Wk.b, Wk.x, Wk.H, lane);   // a failed solve leaves the previous x in place; L overwrites H
        if (lane == 0) Wk.flag = good ? 1 : 0;
      }
      __syncthreads();
      IMARK(6);
      const double* x = Wk.x;   // read from LDS where it is used (a register copy of the 30 unknowns pushed the kernel past 512 VGPRs: 740 B of scratch)
      ok = Wk.flag != 0;
      apply_update_t<RIG>(g, S, x);
      if (LASTFRAME && tid == 0) apply_update_t<RIG>(g, sS1, x + 15);
      __syncthreads();
      IMARK(7);
    }
    IMARK(1);
    // ---- classification (Optimizer.cc:4619-4676 / :5000-5057)
    int bad = 0, inl = 0;
    const float cm = LASTFRAME ? chi2MonoF[it] : chi2MonoKF[it];
    const float chi2close = 1.5f * cm;
    for (int i = tid; i < n; i += 256) {
      if (!hasMP[base + i]) continue;
      const float* o = obs + (base + i) * 3;
      const bool st = !RIG && !(o[2] < 0);
      const int cam = i >= nL ? 1 : 0;
      const double X[3] = {(double)Xw[(base + i) * 3], (double)Xw[(base + i) * 3 + 1], (double)Xw[(base + i) * 3 + 2]};
      double err[3], Xc[3];
      // an outlier's error is taken at the current state, an active edge's at the state of the last linearisation (Sprev) — picked element by
      // element: a reference chosen between the two structs at run time puts both (2 x 360 B) into scratch memory
      VIState Q;
      const bool cur = outlier[base + i] != 0;
#pragma unroll
      for (int k = 0; k < 9; ++k) { Q.Rcw[k] = cur ? S.Rcw[k] : Sprev.Rcw[k]; if (RIG) Q.Rcw1[k] = cur ? S.Rcw1[k] : Sprev.Rcw1[k]; }
#pragma unroll
      for (int k = 0; k < 3; ++k) { Q.tcw[k] = cur ? S.tcw[k] : Sprev.tcw[k]; if (RIG) Q.tcw1[k] = cur ? S.tcw1[k] : Sprev.tcw1[k]; }
      const float chi2 = (float)vis_error_t<RIG>(g, Q, X, o, st, (double)invSigma2[base + i], err, Xc, cam);
      bool isOut;
      if (st) isOut = chi2 > chi2Stereo[it];
      else {
        const bool bClose = closeFlag[base + i] != 0;
        const double r6 = cam ? S.Rcw1[6] : S.Rcw[6], r7 = cam ? S.Rcw1[7] : S.Rcw[7], r8 = cam ? S.Rcw1[8] : S.Rcw[8], tz = cam ? S.tcw1[2] : S.tcw[2];
        const bool depthPos = (r6 * X[0] + r7 * X[1] + r8 * X[2] + tz) > 0.0;
        isOut = (chi2 > cm && !bClose) || (bClose && chi2 > chi2close) || !depthPos;
      }
      outlier[base + i] = isOut ? 1 : 0;
      bad += isOut ? 1 : 0; inl += isOut ? 0 : 1;
    }
    bad = (int)wave_sum((double)bad); inl = (int)wave_sum((double)inl);
    __syncthreads();
    if (lane == 0) { Wk.cnt[wv][0] = bad; Wk.cnt[wv][1] = inl; }
    __syncthreads();
    nBad = Wk.cnt[0][0] + Wk.cnt[1][0] + Wk.cnt[2][0] + Wk.cnt[3][0];
    nInl = Wk.cnt[0][1] + Wk.cnt[1][1] + Wk.cnt[2][1] + Wk.cnt[3][1];
    __syncthreads();
    IMARK(8);
    if (it == 2) robust = false;
    if (nInit + (LASTFRAME ? 4 : 3) < 10) break;   // optimizer.edges().size() < 10
  }

  if (nInl < 30 && !bRecInit) {   // :4683-4707
    int bad = 0;
    for (int i = tid; i < n; i += 256) {
      if (!hasMP[base + i]) continue;
      const float* o = obs + (base + i) * 3;
      const bool st = !RIG && !(o[2] < 0);
      const double X[3] = {(double)Xw[(base + i) * 3], (double)Xw[(base + i) * 3 + 1], (double)Xw[(base + i) * 3 + 2]};
      double err[3], Xc[3];
      const float chi2 = (float)vis_error_t<RIG>(g, S, X, o, st, (double)invSigma2[base + i], err, Xc, i >= nL ? 1 : 0);
      if (chi2 < (st ? 24.f : 18.f)) outlier[base + i] = 0; else ++bad;
    }
    bad = (int)wave_sum((double)bad);
    __syncthreads();
    if (lane == 0) Wk.cnt[wv][0] = bad;
    __syncthreads();
    nBad = Wk.cnt[0][0] + Wk.cnt[1][0] + Wk.cnt[2][0] + Wk.cnt[3][0];
    __syncthreads();
  }

  if (tid == 0) {
    float* s0 = stateIO + 21 * f;
    for (int k = 0; k < 9; ++k) s0[k] = (float)S.Rwb[k];
    for (int k = 0; k < 3; ++k) { s0[9 + k] = (float)S.twb[k]; s0[12 + k] = (float)S.v[k]; s0[15 + k] = (float)S.bg[k]; s0[18 + k] = (float)S.ba[k]; }
    nInliersOut[f] = nInit - nBad;
  }
  IMARK(9);
  if (!prior) return;
  // ---- ConstraintPoseImu for the next frame (:4717-4754 / :5094-5150): un-robustified Hessians at the final state, inliers only.
  // Reference order of the 30 x 30 H: [state 1 (0..14) | frame (15..29)] = the inertial edge's own column order for its first 24.
  double acc[21];
#pragma unroll
  for (int k = 0; k < 21; ++k) acc[k] = 0;
  for (int i = tid; i < n; i += 256) {
    if (!hasMP[base + i] || outlier[base + i]) continue;
    const float* o = obs + (base + i) * 3;
    const bool st = !RIG && !(o[2] < 0);
    const int cam = i >= nL ? 1 : 0;
    const double X[3] = {(double)Xw[(base + i) * 3], (double)Xw[(base + i) * 3 + 1], (double)Xw[(base + i) * 3 + 2]};
    const double info = (double)invSigma2[base + i];
    double err[3], Xc[3], J[18];
    vis_error_t<RIG>(g, S, X, o, st, info, err, Xc, cam);
    vis_jacobian_t<RIG>(g, Xc, st, J, cam);
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int cc = r; cc < 6; ++cc) {
        double h = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) h += J[k * 6 + r] * info * J[k * 6 + cc];   // mono: third row is zero
        acc[q++] += h;
      }
  }
#pragma unroll
  for (int k = 0; k < 21; ++k) acc[k] = wave_sum(acc[k]);
  __syncthreads();
  if (lane == 0) for (int k = 0; k < 21; ++k) Wk.red[wv][k] = acc[k];
  if (tid == 64) inertial_edge(P, S1, S, delta, LASTFRAME, Wk.e, Wk.J);
  if (LASTFRAME && tid == 128) prior_edge(pr, S1, Wk.ep, Wk.Jp);
  __syncthreads();
  for (int k = tid; k < 216; k += 256) { const int r = k / 24, c = k - r * 24; double s = 0; for (int l = 0; l < 9; ++l) s += Wk.InfoI[r * 9 + l] * Wk.J[l * 24 + c]; Wk.OJ[k] = s; }
  if (LASTFRAME) for (int k = tid; k < 225; k += 256) { const int r = k / 15, c = k - r * 15; double s = 0; for (int l = 0; l < 15; ++l) s += Wk.pH[r * 15 + l] * Wk.Jp[l * 15 + c]; Wk.OJp[k] = s; }
  __syncthreads();
  for (int k = tid; k < 900; k += 256) {   // H30 in the reference order
    const int r = k / 30, c = k - r * 30;
    double h = 0;
    if (r < 24 && c < 24) { double s = 0; for (int l = 0; l < 9; ++l) s += Wk.J[l * 24 + r] * Wk.OJ[l * 24 + c]; h += s; }
    const int rb = r % 15, cb = c % 15;
    if (rb >= 9 && cb >= 9 && (rb < 12) == (cb < 12)) {
      const double* I3 = rb < 12 ? Wk.InfoG : Wk.InfoA;
      const double v = I3[(rb - (rb < 12 ? 9 : 12)) * 3 + (cb - (cb < 12 ? 9 : 12))];
      if (LASTFRAME) h += ((r < 15) == (c < 15)) ? v : -v;          // GetHessian(): both vertices
      else if (r >= 15 && c >= 15) h += v;                           // GetHessian2(): the frame's bias only
    }
    if (LASTFRAME && r < 15 && c < 15) { double s = 0; for (int l = 0; l < 15; ++l) s += Wk.Jp[l * 15 + r] * Wk.OJp[l * 15 + c]; h += s; }
    if (r >= 15 && c >= 15 && r < 21 && c < 21) {
      const int a = (r < c ? r : c) - 15, bq = (r < c ? c : r) - 15;
      const int q = a * 6 - a * (a - 1) / 2 + (bq - a);
      h += Wk.red[0][q] + Wk.red[1][q] + Wk.red[2][q] + Wk.red[3][q];
    }
    Wk.H[k] = h;
  }
  __syncthreads();
  double* Hout = prior + (size_t)246 * f + 21;
  if (!LASTFRAME) {
    // GetHessian2 of the inertial edge = its (P2, V2) columns: rows / cols 15..23 of H30; the result is the trailing 15 x 15
    for (int k = tid; k < 225; k += 256) { const int r = k / 15, c = k - r * 15; Wk.Jp[k] = Wk.H[(15 + r) * 30 + 15 + c]; }
    __syncthreads();
  } else {
    // Optimizer::Marginalize(H, 0, 14) (Optimizer.cc:2898-2977): Hcc - Hcp pinv(Hpp) Hpc, singular values <= 1e-6 dropped.
    // All singular values above the threshold (Hpp - 1e-6 I positive definite) <=> the pseudo-inverse is the inverse: LDL^T
    // solves; otherwise the eigen-decomposition path below.
    // Hpp -> Jp (factor), Hpc -> OJp (15 right-hand sides, solved in place column by column)
    for (int k = tid; k < 225; k += 256) { const int r = k / 15, c = k - r * 15; Wk.Jp[k] = 0.5 * (Wk.H[r * 30 + c] + Wk.H[c * 30 + r]); Wk.OJp[k] = Wk.H[r * 30 + 15 + c]; }
    __syncthreads();
    if (tid == 0) {
      // test on a copy (J | OJ hold 432 doubles)
      double* T = Wk.J;
      for (int k = 0; k < 225; ++k) T[k] = Wk.Jp[k];
      for (int k = 0; k < 15; ++k) T[k * 15 + k] -= 1e-6;
      bool pd = true;
      for (int j = 0; j < 15 && pd; ++j) {
        const double d = T[j * 15 + j];
        if (!(d > 0)) { pd = false; break; }
        for (int r = 14; r > j; --r) { const double l = T[r * 15 + j] / d; for (int c = j + 1; c <= r; ++c) T[r * 15 + c] -= l * T[c * 15 + j]; }
      }
      Wk.flag = pd ? 1 : 0;
    }
    __syncthreads();
    if (Wk.flag) {
      // X = Hpp^-1 Hpc: factor once (wave 0), then 15 substitutions
      if (wv == 0) {
        for (int j = 0; j < 15; ++j) {
          WAVE_SYNC();
          const double d = Wk.Jp[j * 15 + j];
          const int m = 14 - j, pairs = m * (m + 1) / 2;
          for (int p = lane; p < pairs; p += 64) {
            int rr = (int)((sqrtf(8.f * (float)p + 1.f) - 1.f) * 0.5f);
            while ((rr + 1) * (rr + 2) / 2 <= p) ++rr;
            while (rr * (rr + 1) / 2 > p) --rr;
            const int cc = p - rr * (rr + 1) / 2;
            const int r = j + 1 + rr, c = j + 1 + cc;
            Wk.Jp[r * 15 + c] -= Wk.Jp[r * 15 + j] * Wk.Jp[c * 15 + j] / d;
          }
          WAVE_SYNC();
          for (int r = j + 1 + lane; r < 15; r += 64) Wk.Jp[r * 15 + j] /= d;
        }
        WAVE_SYNC();
      }
      __syncthreads();
      if (tid < 15) {   // one right-hand side (column tid of Hpc) per thread
        double y[15];
        for (int r = 0; r < 15; ++r) { double s = Wk.OJp[r * 15 + tid]; for (int c = 0; c < r; ++c) s -= Wk.Jp[r * 15 + c] * y[c]; y[r] = s; }
        for (int r = 0; r < 15; ++r) y[r] /= Wk.Jp[r * 15 + r];
        for (int r = 14; r >= 0; --r) { double s = y[r]; for (int c = r + 1; c < 15; ++c) s -= Wk.Jp[c * 15 + r] * y[c]; y[r] = s; }
        for (int r = 0; r < 15; ++r) Wk.OJp[r * 15 + tid] = y[r];
      }
      __syncthreads();
    } else {
      if (tid == 0) {   // pinv by the eigen-decomposition (rare): V diag(1/e, |e| > 1e-6) V^T
        double* A = Wk.J;          // 225 (J | OJ = 432 doubles)
        double* V = Wk.J + 225;    // needs 225: spills into OJ's tail + e/Oe ... keep within J|OJ: 432 < 450 -> use b/x region too
        // 450 doubles needed: J (216) + OJ (216) + e (9) + Oe (9) are contiguous in InertialWork
        for (int k = 0; k < 225; ++k) { A[k] = Wk.Jp[k]; V[k] = 0.0; }
        for (int k = 0; k < 15; ++k) V[k * 15 + k] = 1.0;
        for (int sweep = 0; sweep < 60; ++sweep) {
          double off = 0, diag = 0;
          for (int r = 0; r < 15; ++r) for (int c = 0; c < 15; ++c) { const double t = A[r * 15 + c] * A[r * 15 + c]; if (r == c) diag += t; else off += t; }
          if (off <= 1e-30 * diag) break;
          for (int p = 0; p < 15; ++p)
            for (int q = p + 1; q < 15; ++q) {
              if (A[p * 15 + q] == 0.0) continue;
              const double theta = (A[q * 15 + q] - A[p * 15 + p]) / (2.0 * A[p * 15 + q]);
              const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
              const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
              for (int k = 0; k < 15; ++k) { const double a = A[k * 15 + p], bq = A[k * 15 + q]; A[k * 15 + p] = c * a - s * bq; A[k * 15 + q] = s * a + c * bq; }
              for (int k = 0; k < 15; ++k) { const double a = A[p * 15 + k], bq = A[q * 15 + k]; A[p * 15 + k] = c * a - s * bq; A[q * 15 + k] = s * a + c * bq; }
              for (int k = 0; k < 15; ++k) { const double a = V[k * 15 + p], bq = V[k * 15 + q]; V[k * 15 + p] = c * a - s * bq; V[k * 15 + q] = s * a + c * bq; }
            }
        }
        // Jp <- pinv
        for (int r = 0; r < 15; ++r)
          for (int c = 0; c < 15; ++c) {
            double s = 0;
            for (int k = 0; k < 15; ++k) { const double e = A[k * 15 + k]; if (fabs(e) > 1e-6) s += V[r * 15 + k] * (1.0 / e) * V[c * 15 + k]; }
            Wk.Jp[r * 15 + c] = s;
          }
        // OJp <- pinv * Hpc
        for (int c = 0; c < 15; ++c) {
          double y[15];
          for (int r = 0; r < 15; ++r) { double s = 0; for (int k = 0; k < 15; ++k) s += Wk.Jp[r * 15 + k] * Wk.OJp[k * 15 + c]; y[r] = s; }
          for (int r = 0; r < 15; ++r) Wk.OJp[r * 15 + c] = y[r];
        }
      }
      __syncthreads();
    }
    // Hcc - Hcp X  -> Jp
    double hv = 0;
    if (tid < 225) {
      const int r = tid / 15, c = tid - r * 15;
      double s = 0;
      for (int k = 0; k < 15; ++k) s += Wk.H[(15 + r) * 30 + k] * Wk.OJp[k * 15 + c];
      hv = Wk.H[(15 + r) * 30 + 15 + c] - s;
    }
    __syncthreads();
    if (tid < 225) Wk.Jp[tid] = hv;
    __syncthreads();
  }
  if (tid == 0) clamp_eigenvalues(Wk.Jp, 15, 1e-12, Wk.J, Wk.OJp);   // ConstraintPoseImu's constructor; J | OJ | e | Oe = 450 doubles
  __syncthreads();
  IMARK(10);
  for (int k = tid; k < 225; k += 256) Hout[k] = Wk.Jp[k];
  if (tid == 0) {
    double* out = prior + (size_t)246 * f;
    for (int k = 0; k < 9; ++k) out[k] = S.Rwb[k];
    for (int k = 0; k < 3; ++k) { out[9 + k] = S.twb[k]; out[12 + k] = S.v[k]; out[15 + k] = S.bg[k]; out[18 + k] = S.ba[k]; }
  }
}

}  // namespace

extern "C" {

int morb_imu_preintegrate_batch(morb_optimizer* o, int nseq, const int* d_start, const float* d_acc, const float* d_gyro,
                                const float* d_dt, const float* d_bias, const float* ngaDiag6, const float* walkDiag6,
                                morb_imu_preintegrated* d_out, void* stream) {
  MORB_REQUIRE(o && d_start && d_acc && d_gyro && d_dt && d_bias && ngaDiag6 && walkDiag6 && d_out, MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nseq > 0, MORB_ERR_INVALID, "nseq must be positive");
  MORB_ENTER(st, o, stream);
  morb_imu_preintegrated calib;
  memset(&calib, 0, sizeof calib);
  memcpy(calib.nga, ngaDiag6, sizeof(float) * 6);
  memcpy(calib.ngaWalk, walkDiag6, sizeof(float) * 6);
  hipLaunchKernelGGL(k_imu_preintegrate, dim3(nseq), dim3(64), 0, st, nseq, d_start, d_acc, d_gyro, d_dt, d_bias, calib, d_out);
  MORB_HIP_CHECK(hipGetLastError());
  return MORB_OK;
}

static int launch_pose_inertial(bool lastFrame, morb_optimizer* o, int nframes, int cap, const int* d_count, const uint8_t* d_hasMP,
                                const float* d_obs, const float* d_invSigma2, const float* d_Xw, const uint8_t* d_close, float fx,
                                float fy, float cx, float cy, float bf, const float* Tbc12, const float* d_state1,
                                const morb_imu_preintegrated* d_pre, const morb_imu_preintegrated* d_preKF,
                                const double* d_prevPrior, int bRecInit, float* d_state, uint8_t* d_outlier, int* d_nInliers,
                                double* d_prior, void* stream, const int* d_nLeft = nullptr, const float* rig28 = nullptr) {
  MORB_REQUIRE(o && d_hasMP && d_obs && d_invSigma2 && d_Xw && d_close && Tbc12 && d_state1 && d_pre && d_state && d_outlier && d_nInliers,
               MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(!lastFrame || (d_preKF && d_prevPrior), MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(!rig28 || d_nLeft, MORB_ERR_INVALID, "a fisheye rig needs d_nLeft");
  MORB_REQUIRE(nframes > 0 && cap > 0, MORB_ERR_INVALID, "bad sizes");
  MORB_ENTER(st, o, stream);
  CamGeom g;
  make_geom(Tbc12, fx, fy, cx, cy, bf, rig28, g);
  const size_t edgeLds = (size_t)cap * 32;   // the active visual edges of a frame, eight floats each
  // (round 5 refused frames whose list does not fit the LDS; now they take the same kernel with the list in a global spill buffer of the handle)
  const bool spill = edgeLds + sizeof(InertialWork) + 1024 > 160 * 1024;
  float* gEdge = nullptr;
  if (spill) { const int rc = grow(o->spill, (size_t)nframes * cap * 8, &gEdge); if (rc != MORB_OK) return rc; }
#define MORB_LAUNCH_PI2(LF, RG, GE)                                                                                                  \
  do {                                                                                                                               \
    const size_t lds_ = GE ? 0 : edgeLds;                                                                                            \
    MORB_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pose_inertial<LF, RG, GE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_)); \
    hipLaunchKernelGGL((k_pose_inertial<LF, RG, GE>), dim3(nframes), dim3(256), lds_, st, cap, d_count, d_hasMP, d_obs, d_invSigma2, d_Xw, d_close, \
                       g, d_state1, d_pre, d_preKF, d_prevPrior, d_nLeft, bRecInit, d_state, d_outlier, d_nInliers, d_prior, gEdge);          \
  } while (0)
#define MORB_LAUNCH_PI(LF, RG) do { if (spill) MORB_LAUNCH_PI2(LF, RG, true); else MORB_LAUNCH_PI2(LF, RG, false); } while (0)
  if (lastFrame) { if (rig28) MORB_LAUNCH_PI(true, true); else MORB_LAUNCH_PI(true, false); }
  else { if (rig28) MORB_LAUNCH_PI(false, true); else MORB_LAUNCH_PI(false, false); }
#undef MORB_LAUNCH_PI2
#undef MORB_LAUNCH_PI
  MORB_HIP_CHECK(hipGetLastError());
  return MORB_OK;
}

int morb_pose_inertial_optimization_last_keyframe_batch(morb_optimizer* o, int nframes, int cap, const int* d_count,
                                                        const uint8_t* d_hasMP, const float* d_obs, const float* d_invSigma2,
                                                        const float* d_Xw, const uint8_t* d_close, float fx, float fy, float cx,
                                                        float cy, float bf, const float* Tbc12, const float* d_kfState,
                                                        const morb_imu_preintegrated* d_pre, int bRecInit, float* d_state,
                                                        uint8_t* d_outlier, int* d_nInliers, double* d_prior, void* stream) {
  return launch_pose_inertial(false, o, nframes, cap, d_count, d_hasMP, d_obs, d_invSigma2, d_Xw, d_close, fx, fy, cx, cy, bf, Tbc12,
                              d_kfState, d_pre, nullptr, nullptr, bRecInit, d_state, d_outlier, d_nInliers, d_prior, stream);
}

int morb_pose_inertial_optimization_last_frame_batch(morb_optimizer* o, int nframes, int cap, const int* d_count,
                                                     const uint8_t* d_hasMP, const float* d_obs, const float* d_invSigma2,
                                                     const float* d_Xw, const uint8_t* d_close, float fx, float fy, float cx, float cy,
                                                     float bf, const float* Tbc12, const float* d_prevState,
                                                     const morb_imu_preintegrated* d_preFrame, const morb_imu_preintegrated* d_preKF,
                                                     const double* d_prevPrior, int bRecInit, float* d_state, uint8_t* d_outlier,
                                                     int* d_nInliers, double* d_prior, void* stream) {
  return launch_pose_inertial(true, o, nframes, cap, d_count, d_hasMP, d_obs, d_invSigma2, d_Xw, d_close, fx, fy, cx, cy, bf, Tbc12,
                              d_prevState, d_preFrame, d_preKF, d_prevPrior, bRecInit, d_state, d_outlier, d_nInliers, d_prior, stream);
}

int morb_pose_inertial_optimization_last_keyframe_fisheye_batch(morb_optimizer* o, int nframes, int cap, const int* d_count, const int* d_nLeft,
                                                                const uint8_t* d_hasMP, const float* d_obs, const float* d_invSigma2,
                                                                const float* d_Xw, const uint8_t* d_close, const float* rig28,
                                                                const float* Tbc12, const float* d_kfState,
                                                                const morb_imu_preintegrated* d_pre, int bRecInit, float* d_state,
                                                                uint8_t* d_outlier, int* d_nInliers, double* d_prior, void* stream) {
  MORB_REQUIRE(rig28 && d_nLeft, MORB_ERR_INVALID, "NULL argument");
  return launch_pose_inertial(false, o, nframes, cap, d_count, d_hasMP, d_obs, d_invSigma2, d_Xw, d_close, 0, 0, 0, 0, 0, Tbc12, d_kfState, d_pre,
                              nullptr, nullptr, bRecInit, d_state, d_outlier, d_nInliers, d_prior, stream, d_nLeft, rig28);
}

int morb_pose_inertial_optimization_last_frame_fisheye_batch(morb_optimizer* o, int nframes, int cap, const int* d_count, const int* d_nLeft,
                                                             const uint8_t* d_hasMP, const float* d_obs, const float* d_invSigma2,
                                                             const float* d_Xw, const uint8_t* d_close, const float* rig28, const float* Tbc12,
                                                             const float* d_prevState, const morb_imu_preintegrated* d_preFrame,
                                                             const morb_imu_preintegrated* d_preKF, const double* d_prevPrior, int bRecInit,
                                                             float* d_state, uint8_t* d_outlier, int* d_nInliers, double* d_prior,
                                                             void* stream) {
  MORB_REQUIRE(rig28 && d_nLeft, MORB_ERR_INVALID, "NULL argument");
  return launch_pose_inertial(true, o, nframes, cap, d_count, d_hasMP, d_obs, d_invSigma2, d_Xw, d_close, 0, 0, 0, 0, 0, Tbc12, d_prevState,
                              d_preFrame, d_preKF, d_prevPrior, bRecInit, d_state, d_outlier, d_nInliers, d_prior, stream, d_nLeft, rig28);
}

#ifdef MORB_INERTIAL_TIMING
int morb_inertial_timing(unsigned long long* out, int reset) {
  if (reset) { unsigned long long z[16] = {0}; MORB_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_inertialPhase), z, sizeof(z))); return 0; }
  MORB_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_inertialPhase), 16 * sizeof(unsigned long long)));
  return 0;
}
#endif

}  // extern "C"
