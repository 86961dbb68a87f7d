// The optimizer handle and Optimizer::PoseOptimization (reference src/Optimizer.cc:762-1051) for MI355X (gfx950), device-resident:
// g2o's OptimizationAlgorithmLevenberg (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-194) over
// BlockSolver_6_3 (core/block_solver.hpp:354-590) with the reference's edges (src/OptimizableTypes.cpp,
// g2o/types/types_six_dof_expmap.cpp), restated as a batched kernel: one 256-thread workgroup per frame, the whole LM
// schedule (4 robust / outlier rounds) inside ONE launch per batch; residual + Jacobian + J^T W J per edge, reduced in a
// fixed order (27 doubles, DPP wave sums) -> deterministic; the 6x6 system is solved in registers.
// Optimizer::LocalBundleAdjustment, on the same handle and the same device helpers (optimizer_device.h), is local_ba.hip.
// All arithmetic is FP64 like g2o; the reference's float leaks (float camera parameters, `const float invz` in
// the stereo projection, float Huber deltas, float chi2 tests) are reproduced.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <memory>

#include "common.h"
#include "internal_abi.h"
#include "dense_ldlt.h"
#include "optimizer_device.h"

using namespace morb;

namespace {

// Wave totals of 28 doubles at once, written to out[0 .. 27] (LDS).  Two butterfly steps on gfx950's v_permlane32_swap / v_permlane16_swap fold the
// values four to a register — after them row r (16 lanes) of register g holds partial sums of value 4 g + {0, 2, 1, 3}[r]
// (tools/micro/permlane_swap.hip prints the operand layout) — then a row total is sixteen v_fmac_f64_dpp row_newbcast (dense_ldlt.h) for four values together.
// ~200 instruction slots instead of ~1200 for 28 six-step DPP reductions: a third of k_pose_opt's iteration, whose waves are alone on their SIMDs.
// Fixed order (deterministic); not the order of sum_f64 (the tree-sum mode of PoseOptimization is the only caller).
__device__ __forceinline__ double swap_add_f64(double a, double b, bool rows16) {
  const unsigned long long ua = (unsigned long long)__double_as_longlong(a), ub = (unsigned long long)__double_as_longlong(b);
  unsigned lo0, lo1, hi0, hi1;
  if (rows16) {
    auto l = __builtin_amdgcn_permlane16_swap((unsigned)ua, (unsigned)ub, false, false); lo0 = l[0]; lo1 = l[1];
    auto h = __builtin_amdgcn_permlane16_swap((unsigned)(ua >> 32), (unsigned)(ub >> 32), false, false); hi0 = h[0]; hi1 = h[1];
  } else {
    auto l = __builtin_amdgcn_permlane32_swap((unsigned)ua, (unsigned)ub, false, false); lo0 = l[0]; lo1 = l[1];
    auto h = __builtin_amdgcn_permlane32_swap((unsigned)(ua >> 32), (unsigned)(ub >> 32), false, false); hi0 = h[0]; hi1 = h[1];
  }
  return __longlong_as_double((long long)(((unsigned long long)hi0 << 32) | lo0)) + __longlong_as_double((long long)(((unsigned long long)hi1 << 32) | lo1));
}
template <int K>
__device__ __forceinline__ void row_total_step(double& acc, double v, double minusOne) {
  if constexpr (K < 16) { morbdense::fnma_row_bcast_f64<K, K == 0>(acc, v, minusOne); row_total_step<K + 1>(acc, v, minusOne); }
}
__device__ __forceinline__ void wave_sum28_to(const double (&v)[28], double* __restrict__ out, int lane) {
  double c[14], d[7];
#pragma unroll
  for (int p = 0; p < 14; ++p) c[p] = swap_add_f64(v[2 * p], v[2 * p + 1], false);   // lanes 0 .. 31: value 2 p, lanes 32 .. 63: value 2 p + 1
#pragma unroll
  for (int g = 0; g < 7; ++g) d[g] = swap_add_f64(c[2 * g], c[2 * g + 1], true);      // rows 0 .. 3: values 4 g, 4 g + 2, 4 g + 1, 4 g + 3
  const double minusOne = -1.0;
  const int row = lane >> 4, idx = ((row & 1) << 1) | (row >> 1);
#pragma unroll
  for (int g = 0; g < 7; ++g) {
    double tot = 0.0;
    row_total_step<0>(tot, d[g], minusOne);   // tot += lane k of the row, k = 0 .. 15, in that order: every lane of the row ends with the row's total
    if ((lane & 15) == 0) out[4 * g + idx] = tot;
  }
}

// LDL^T solve of an n x n SPD system held in registers/local arrays (n = 6)
__device__ __forceinline__ bool ldlt6(const double* Hin, const double* rhs, double* x) {
  // (every loop fully unrolled: an index that is not a compile-time constant puts the arrays into scratch memory, and the solve sits on
  // the critical path of every LM iteration)
  double A[36], D[6];
#pragma unroll
  for (int i = 0; i < 36; ++i) A[i] = Hin[i];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[j * 6 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= A[j * 6 + k] * A[j * 6 + k] * D[k];
    ok = ok && (d > 0);   // LinearSolverDense: _cholesky.isPositive() (the factorisation runs on; the caller discards x)
    D[j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i * 6 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= A[i * 6 + k] * A[j * 6 + k] * D[k];
      A[i * 6 + j] = s / d;
    }
  }
  if (!ok) return false;
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    y[i] = rhs[i];
#pragma unroll
    for (int k = 0; k < i; ++k) y[i] -= A[i * 6 + k] * y[k];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) y[i] /= D[i];
#pragma unroll
  for (int i = 5; i >= 0; --i) {
#pragma unroll
    for (int k = i + 1; k < 6; ++k) y[i] -= A[k * 6 + i] * y[k];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = y[i];
  return true;
}

// unary edge of PoseOptimization: residual (returns chi2, sets st = "3-D stereo residual") ...
template <bool FISH>
__device__ __forceinline__ double pose_edge_error(const Cam& cam, const Rig& rig, const SE3& P, const SE3& Pr, bool right,
                                                  const double* X, const float* o, double info, double* err, bool& st,
                                                  double* xc) {
  se3_map(P, X, xc);
  if (!FISH) {
    st = !(o[2] < 0);
    return edge_error(cam, st, xc, o, info, err);
  }
  st = false;
  double uv[2];
  if (!right) morbcam::kb8_project_d(rig.kbL, xc, uv);                       // EdgeSE3ProjectXYZOnlyPose, pCamera = left KB8
  else { double xr[3]; se3_map(Pr, X, xr); morbcam::kb8_project_d(rig.kbR, xr, uv); }   // ...ToBody: (mTrl * T).map(Xw)
  err[0] = (double)o[0] - uv[0]; err[1] = (double)o[1] - uv[1]; err[2] = 0;
  return err[0] * (info * err[0]) + err[1] * (info * err[1]);
}
// ... and its 2x6 / 3x6 Jacobian w.r.t. the pose
template <bool FISH>
__device__ __forceinline__ void pose_edge_jac(const Cam& cam, const Rig& rig, bool right, bool st, const double* xc, double* Jp) {
  if (!FISH) { jac_pose(cam, st, true, xc, Jp); return; }
  const double x = xc[0], y = xc[1], z = xc[2];
  double pj[6], pjM[6];
  if (!right) {
    morbcam::kb8_project_jac(rig.kbL, xc, pj);
    for (int k = 0; k < 6; ++k) pjM[k] = pj[k];
  } else {  // -projectJac(X_r) * R_rl * SE3deriv(X_l), X_r = mTrl.map(T.map(Xw))  (OptimizableTypes.cpp:88-104)
    double xr[3], M[9];
    se3_map(rig.Trl, xc, xr);
    morbcam::kb8_project_jac(rig.kbR, xr, pj);
    q_to_R(rig.Trl.q, M);
    for (int r = 0; r < 2; ++r)
      for (int c = 0; c < 3; ++c) pjM[r * 3 + c] = pj[r * 3] * M[c] + pj[r * 3 + 1] * M[3 + c] + pj[r * 3 + 2] * M[6 + c];
  }
  for (int r = 0; r < 2; ++r) {
    const double a = pjM[r * 3], b = pjM[r * 3 + 1], c = pjM[r * 3 + 2];
    Jp[r * 6 + 0] = -(b * -z + c * y); Jp[r * 6 + 1] = -(a * z + c * -x); Jp[r * 6 + 2] = -(a * -y + b * x);
    Jp[r * 6 + 3] = -a; Jp[r * 6 + 4] = -b; Jp[r * 6 + 5] = -c;
  }
  for (int k = 12; k < 18; ++k) Jp[k] = 0;
}

// =====================================================================================================
// PoseOptimization: one workgroup per frame
// =====================================================================================================
// ORDERED: every sum over the edges (the 21 + 6 entries of H and b, the robustified chi2) is taken in EDGE ORDER, one addition after the
// other, like g2o's sequential loop over its id-sorted active edges (sparse_optimizer.cpp:482-487, block_solver.hpp:502-560) and like the oracle:
// near convergence rho = dChi2 / scale is ~0 and its sign — an LM decision — follows the last bits of those sums.  A strided partial sum per
// thread + a tree gives other last bits (observed: one trial more or less in one of nine problems).  Edges are taken 256 at a time: every
// thread writes its edge's 28 contributions to LDS (an inactive edge: exact zeros, which leave a floating-point sum unchanged), lanes 0 .. 27
// of wave 0 add their entry's 256 values in order.  A chain of dependent FP64 additions per sum: 0.68 ms instead of 0.43 ms per 256 frames of
// 600 edges (tools/pose_opt_modes.py; round 4's figures — round 5's k_pose_opt2 runs the ordered sums on the matrix core: 0.41 against 0.40 ms, and the
// edge-order mode became the default).
#ifndef MORB_PO_NT
#define MORB_PO_NT 256   // threads per frame of PoseOptimization's default (tree-sum) mode
#endif
constexpr int PO_PITCH = 29;   // doubles per edge row of the contribution buffer (28 used)
// tot + p[0] + p[STRIDE] + ... (m terms, m wave-uniform, added strictly in that order): sixteen LDS reads in flight, then their sixteen additions
// — one read per addition made the chain ~100 cycles per term — and no test inside the full batches (a `if (e + k < m)` per addition, although
// uniform, cost the lone wave four instruction slots per term instead of one); the reads of the last, partial batch stay inside the 256-row buffer
template <int STRIDE>
__device__ __forceinline__ double ordered_add(double tot, const double* __restrict__ p, int m) {
  int e = 0;
  for (; e + 16 <= m; e += 16) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = p[(e + k) * STRIDE];
#pragma unroll
    for (int k = 0; k < 16; ++k) tot += v[k];
  }
  if (e < m) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = p[(e + k) * STRIDE];   // (rows beyond m hold an earlier chunk's values: not added)
#pragma unroll
    for (int k = 0; k < 16; ++k) if (e + k < m) tot += v[k];
  }
  return tot;
}
// The same sum, software-pipelined for a wave that is (nearly) alone on its SIMD.  Such a wave issues an instruction every ~6 cycles whatever it is and a
// dependent v_add_f64 every ~12 (tools/micro/f64_chain.hip -> profiles/r05/f64_chain_cycles_per_term.txt), so a term costs 12 cycles + 6 per other
// instruction: the next eight rows are REQUESTED before the current eight are added (the compiler had placed every batch's reads directly in front of
// their use: a full LDS round trip per batch, ~23 cycles per term); empty asm statements that carry the running sum and clobber memory pin that order
// (17); 32 terms per loop trip (two register sets, no copies).  Interleaving one read per two additions measured 20 in the micro-benchmark: reads do not
// hide in an addition's shadow.  ROWS = rows of the buffer (a multiple of 8): reads never leave it; rows >= m are read and not added.
template <int STRIDE, int ROWS>
__device__ __forceinline__ double ordered_add_pipe(double tot, const double* __restrict__ p, int m) {
  static_assert(ROWS % 8 == 0, "whole batches");
  double v[8], w[8];
#define MORB_LOAD8(dst, row)                                                   \
  do {                                                                         \
    const int r_ = (row) <= ROWS - 8 ? (row) : ROWS - 8;                       \
    _Pragma("unroll") for (int k = 0; k < 8; ++k) dst[k] = p[(r_ + k) * STRIDE]; \
    asm volatile("" : "+v"(tot) : : "memory");                                 \
  } while (0)
#define MORB_ADD8(src)                                                                                                                       \
  do {                                                                                                                                       \
    _Pragma("unroll") for (int k = 0; k < 8; ++k) tot += src[k];                                                                             \
    asm volatile("" : "+v"(tot) : : "memory");                                                                                               \
  } while (0)
  MORB_LOAD8(v, 0);
  int e = 0;
  for (; e + 32 <= m; e += 32) {
    MORB_LOAD8(w, e + 8);  MORB_ADD8(v);
    MORB_LOAD8(v, e + 16); MORB_ADD8(w);
    MORB_LOAD8(w, e + 24); MORB_ADD8(v);
    MORB_LOAD8(v, e + 32); MORB_ADD8(w);
  }
  for (; e + 8 <= m; e += 8) {   // (v holds rows e .. e + 7)
    MORB_LOAD8(w, e + 8);
    MORB_ADD8(v);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = w[k];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) if (e + k < m) tot += v[k];
#undef MORB_LOAD8
#undef MORB_ADD8
  return tot;
}
// The same sums on the FP64 matrix core.  v_mfma_f64_4x4x4_4b_f64 computes D[b][i][j] = C[b][i][j] + sum_k A[b][i][k] B[b][k][j] for four 4 x 4
// blocks b; on gfx950 the four products are added one after the other, k = 0 .. 3, each sum rounded to double — with B = 1 that is
// (((c + a0) + a1) + a2) + a3, bit for bit what four dependent v_add_f64 produce (tools/micro/mfma_chain.hip: 262 144 random accumulations with
// mixed signs, magnitudes 2^-30 .. 2^30 and near-total cancellation, all equal; k_mfma_order_selftest repeats the check when a handle is created and
// the VALU chain above stays as the form a device that fails it would run).  One instruction therefore advances 16 independent ordered sums
// (b, i) by FOUR edges in 4 passes; a dependent MFMA issues after ~25 cycles: ~7 cycles per edge with the 28 sums in two waves (16 + 12) where the
// v_add_f64 chain measured 14 - 17 inside this kernel (profiles/r05/README.md).
// Layout (found with one-hot operands): A lane = 16 k + 4 b + i, B lane = 16 k + 4 b + j, C / D lane = 16 i + 4 b + j.  Lane l of the summing wave
// reads entry (l & 15) [+ 16 in the second wave] of edge row e + (l >> 4); sum c (< 16) comes out in lanes 16 (c & 3) + 4 (c >> 2) + j.
// The rows [m, m16) have been zeroed by the workers (x + 0.0 is exact and the running sums are never -0.0).  ROWS is a multiple of 16.
// One accumulator (16 sums) per wave: a dependent MFMA every ~25 cycles, the reads of the rows 32 ahead in its shadow.  Two waves on two SIMDs carry the
// 28 sums at ~7 cycles per edge (sC16 = sC + 16 x the wave's index; ROWS is a multiple of 32).  (Both accumulators interleaved in one wave: 11 cycles per edge.)
template <int STRIDE, int ROWS>
__device__ __forceinline__ void ordered_add_mfma1(double& d, const double* __restrict__ sC16, int lane, int m16) {
  static_assert(ROWS % 32 == 0, "whole batches");
  const double* p = sC16 + (lane >> 4) * STRIDE + (lane & 15);
  double r[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) r[t] = p[4 * t * STRIDE];
  asm volatile("" : "+v"(d) : : "memory");
  int e = 0;
  for (; e + 32 <= m16; e += 32) {
    const double* q = p + (e + 32 <= ROWS - 32 ? e + 32 : ROWS - 32) * STRIDE;   // (reads never leave the buffer)
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      d = __builtin_amdgcn_mfma_f64_4x4x4f64(r[t], 1.0, d, 0, 0, 0);
      r[t] = q[4 * t * STRIDE];
      asm volatile("" : "+v"(d) : : "memory");
    }
  }
  if (e < m16) {
#pragma unroll
    for (int t = 0; t < 4; ++t) d = __builtin_amdgcn_mfma_f64_4x4x4f64(r[t], 1.0, d, 0, 0, 0);
  }
}
// one wave: `rounds` accumulations of four pseudo-random terms per lane group through the matrix core and through dependent v_add_f64; *bad counts
// the results that differ in any bit
__global__ __launch_bounds__(64) void k_mfma_order_selftest(int rounds, int* __restrict__ bad) {
  const int lane = threadIdx.x;
  unsigned long long x = 0x9E3779B97F4A7C15ull * (unsigned long long)(lane + 1);
  auto next = [&]() {   // xorshift64* -> a double with a random sign, a full mantissa and an exponent in [-30, 30]
    x ^= x >> 12; x ^= x << 25; x ^= x >> 27;
    const unsigned long long r = x * 0x2545F4914F6CDD1Dull;
    const unsigned long long expo = 1023ull - 30ull + (r >> 52) % 61ull;
    return __longlong_as_double((long long)((r & 0x800FFFFFFFFFFFFFull) | (expo << 52)));
  };
  const int c16 = 4 * ((lane >> 2) & 3) + (lane >> 4);   // the sum this lane's C / D register holds
  const int s16 = lane & 15, dl = 16 * (s16 & 3) + 4 * (s16 >> 2);   // the sum this lane's A register feeds, and a D lane that holds it
  int nbad = 0;
  double c = 0.0;
  for (int r = 0; r < rounds; ++r) {
    double a = next();
    const double cs = __shfl(c, dl), a0s = __shfl(a, s16);
    if ((r & 3) == 1 && (lane >> 4) == 1) a = -(cs + a0s) * (1.0 + 0x1p-40 * (double)(x & 1023));   // the second term nearly cancels the running sum
    double ref = c;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const double ak = __shfl(a, c16 + 16 * k); asm volatile("v_add_f64 %0, %0, %1" : "+v"(ref) : "v"(ak)); }
    c = __builtin_amdgcn_mfma_f64_4x4x4f64(a, 1.0, c, 0, 0, 0);
    nbad += __double_as_longlong(c) != __double_as_longlong(ref);
    if ((r & 15) == 15) c = next();   // a fresh running sum now and then
  }
  if (nbad) atomicAdd(bad, nbad);
}
#ifdef MORB_PO_TRACE
__device__ double g_poTrace[6 * 520];
__device__ int g_poTraceN;
extern "C" int morb_po_trace(double* out, int* n) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_poTrace), sizeof(double) * 6 * 520); (void)hipMemcpyFromSymbol(n, HIP_SYMBOL(g_poTraceN), sizeof(int)); const int z = 0; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_poTraceN), &z, sizeof z); return 0; }
#endif
template <bool FISH, bool ORDERED, int NT>
__global__ __launch_bounds__(NT) void k_pose_opt(int cap, const int* __restrict__ count, const uint8_t* __restrict__ hasMP,
                                                  const float* __restrict__ obs, const float* __restrict__ invSigma2,
                                                  const float* __restrict__ Xw, Cam cam, Rig rig, const int* __restrict__ nLeft,
                                                  float* __restrict__ poseIO, uint8_t* __restrict__ outlier,
                                                  int* __restrict__ nInliers, int* __restrict__ stats) {
  constexpr int NW = NT / 64;
  static_assert(!ORDERED || NT == 256, "the edge-order mode takes its edges 256 at a time");
  __shared__ double red[NW];
  __shared__ double sH[NW][28];
  __shared__ double sC[ORDERED ? 256 * PO_PITCH : 1];   // [edge of the chunk][entry]
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = count ? count[f] : cap;
  const size_t base = (size_t)f * cap;
  const double deltaMono = (double)(float)sqrt(5.991), deltaStereo = (double)(float)sqrt(7.815);

  int nInit = 0;
  for (int i = tid; i < n; i += NT) {
    if (hasMP[base + i]) { ++nInit; outlier[base + i] = 0; }
  }
  nInit = (int)block_sum_d<NW>((double)nInit, red);
  if (nInit < 3) {  // Optimizer.cc:951
    if (tid == 0) { nInliers[f] = 0; if (stats) { stats[2 * f] = 0; stats[2 * f + 1] = 0; } }
    return;
  }
  const SE3 T0 = se3_from_float(poseIO + 7 * f);
  SE3 T = T0, Teval = T0;
  bool robust = true;
  int nBadEdges = 0, outerIts = 0, trials = 0;

  const int nL = FISH ? nLeft[f] : n;   // features >= nL are right-camera observations (fisheye rig)
  // robustified chi2 of the active edges at pose P
  auto chi2Active = [&](const SE3& P) -> double {
    const SE3 Pr = FISH ? se3_mul(rig.Trl, P) : P;
    double s = 0;
    if (ORDERED) {
      double tot = 0;
      for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + tid;
        double c = 0;
        if (i < n && hasMP[base + i] && !outlier[base + i]) {
          const float* o = obs + (base + i) * 3;
          const double X[3] = {(double)Xw[(base + i) * 3], (double)Xw[(base + i) * 3 + 1], (double)Xw[(base + i) * 3 + 2]};
          double xc[3], err[3], w;
          bool st;
          c = pose_edge_error<FISH>(cam, rig, P, Pr, FISH && i >= nL, X, o, (double)invSigma2[base + i], err, st, xc);
          if (robust) c = huber(st ? deltaStereo : deltaMono, c, &w);
        }
        sC[tid] = c;
        __syncthreads();
        if (tid == 0) tot = ordered_add<1>(tot, sC, n - c0 < 256 ? n - c0 : 256);
        __syncthreads();
      }
      if (tid == 0) red[0] = tot;
      __syncthreads();
      tot = red[0];
      __syncthreads();
      return tot;
    }
    for (int i = tid; i < n; i += NT) {
      if (!hasMP[base + i] || outlier[base + i]) continue;
      const float* o = obs + (base + i) * 3;
      const double X[3] = {(double)Xw[(base + i) * 3], (double)Xw[(base + i) * 3 + 1], (double)Xw[(base + i) * 3 + 2]};
      double xc[3], err[3], w;
      bool st;
      double c = pose_edge_error<FISH>(cam, rig, P, Pr, FISH && i >= nL, X, o, (double)invSigma2[base + i], err, st, xc);
      if (robust) c = huber(st ? deltaStereo : deltaMono, c, &w);
      s += c;
    }
    return block_sum_d<NW>(s, red);
  };

  for (int it = 0; it < 4; ++it) {
    T = T0;  // vSE3->setEstimate(pFrame->GetPose()) (:962-964)
    // ---- optimizer.optimize(10) ----
    double lambda = 0, ni = 2;
    int nBad = 0;
    for (int iter = 0; iter < 10; ++iter) {
      ++outerIts;
      // computeActiveErrors + activeRobustChi2 + buildSystem in one pass
      const SE3 Tr = FISH ? se3_mul(rig.Trl, T) : T;
      double acc[28];
#pragma unroll
      for (int k = 0; k < 28; ++k) acc[k] = 0;
      if (ORDERED) {
        double tot = 0;   // lanes 0 .. 27 of wave 0: entry `lane` (H upper triangle 0 .. 20, b 21 .. 26, chi2 27)
        for (int c0 = 0; c0 < n; c0 += 256) {
          const int i = c0 + tid;
          double con[28];
#pragma unroll
          for (int k = 0; k < 28; ++k) con[k] = 0;
          if (i < n && hasMP[base + i] && !outlier[base + i]) {
            const float* o = obs + (base + i) * 3;
            const double X[3] = {(double)Xw[(base + i) * 3], (double)Xw[(base + i) * 3 + 1], (double)Xw[(base + i) * 3 + 2]};
            double xc[3], err[3], Jp[18], w = 1.0;
            bool st;
            const double info = (double)invSigma2[base + i];
            const bool right = FISH && i >= nL;
            double c = pose_edge_error<FISH>(cam, rig, T, Tr, right, X, o, info, err, st, xc);
            if (robust) c = huber(st ? deltaStereo : deltaMono, c, &w);
            con[27] = c;
            pose_edge_jac<FISH>(cam, rig, right, st, xc, Jp);
            // g2o's own expressions (base_unary_edge.hpp:54-66): omega_r = -Omega e (then * rho'), b += J^T omega_r, H += J^T (rho' Omega) J
            const double wr[3] = {-info * err[0] * w, -info * err[1] * w, -info * err[2] * w};
            const double wo = w * info;
            int q = 0;
#pragma unroll
            for (int r = 0; r < 6; ++r) {
              double bb = 0;
#pragma unroll
              for (int k = 0; k < 3; ++k) bb += Jp[k * 6 + r] * wr[k];   // (mono: row 2 and err[2] are zero)
              con[21 + r] = bb;
#pragma unroll
              for (int cc = 0; cc <= r; ++cc) {   // the LOWER triangle, (J_r w Omega) J_c as Eigen forms it: LinearSolverDense's LDLT reads that triangle
                double h = 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) h += Jp[k * 6 + r] * wo * Jp[k * 6 + cc];
                con[q++] = h;
              }
            }
          }
#pragma unroll
          for (int k = 0; k < 28; ++k) sC[tid * PO_PITCH + k] = con[k];
          __syncthreads();
          if (tid < 28) tot = ordered_add<PO_PITCH>(tot, sC + tid, n - c0 < 256 ? n - c0 : 256);
          __syncthreads();
        }
        if (tid < 28) sH[0][tid] = tot;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 28; ++k) acc[k] = sH[0][k];
        __syncthreads();
      } else
      for (int i = tid; i < n; i += NT) {
        if (!hasMP[base + i] || outlier[base + i]) continue;
        const float* o = obs + (base + i) * 3;
        const double X[3] = {(double)Xw[(base + i) * 3], (double)Xw[(base + i) * 3 + 1], (double)Xw[(base + i) * 3 + 2]};
        double xc[3], err[3], Jp[18], w = 1.0;
        bool st;
        const double info = (double)invSigma2[base + i];
        const bool right = FISH && i >= nL;
        double c = pose_edge_error<FISH>(cam, rig, T, Tr, right, X, o, info, err, st, xc);
        if (robust) c = huber(st ? deltaStereo : deltaMono, c, &w);
        acc[27] += c;
        pose_edge_jac<FISH>(cam, rig, right, st, xc, Jp);
        const double wo = w * info;
        int q = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          double bb = 0;
#pragma unroll
          for (int k = 0; k < 3; ++k) bb += Jp[k * 6 + r] * (info * err[k]);   // mono: row 2 and err[2] are zero; a runtime bound would push Jp into scratch memory
          acc[21 + r] -= w * bb;  // b -= rho' * J^T * Omega * e  (base_unary_edge.hpp:61)
#pragma unroll
          for (int cc = 0; cc <= r; ++cc) {   // the LOWER triangle, (J_r w Omega) J_c as Eigen forms it: LinearSolverDense's LDLT reads that triangle
            double h = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) h += Jp[k * 6 + r] * wo * Jp[k * 6 + cc];
            acc[q++] += h;
          }
        }
      }
      if (!ORDERED) {
        // (the chi2 entry keeps the reduction order of chi2Active's block sum: rho compares the two, and near convergence their difference is of the
        // size of a summation-order effect)
        const double chiW = wave_sum_d(acc[27]);
        acc[27] = 0;
        __syncthreads();
        wave_sum28_to(acc, sH[wv], lane);
        if (lane == 0) sH[wv][27] = chiW;   // (a later instruction than the zero lane 48 just stored there: LDS keeps a wave's instructions in order)
        __syncthreads();
      }
      double H[36], b[6];
      {
        double tot[28];
        for (int k = 0; k < 28; ++k) {
          if (ORDERED) tot[k] = acc[k];
          else { double t = sH[0][k]; for (int w = 1; w < NW; ++w) t += sH[w][k]; tot[k] = t; }   // ((s0 + s1) + s2) + s3 ...: the order of the 4-wave form
        }
        int q = 0;
        for (int r = 0; r < 6; ++r) for (int cc = 0; cc <= r; ++cc) { H[r * 6 + cc] = tot[q]; H[cc * 6 + r] = tot[q]; ++q; }   // (the solve reads the lower triangle)
        for (int r = 0; r < 6; ++r) b[r] = tot[21 + r];
        acc[27] = tot[27];
      }
#ifdef MORB_PO_TRACE
      if (f == 0 && tid == 0 && outerIts == 1) { double* t = g_poTrace + 6 * 504; for (int k = 0; k < 36; ++k) t[k] = H[k]; for (int k = 0; k < 6; ++k) t[36 + k] = b[k]; }
#endif
      double currentChi = acc[27];
      const double iniChi = currentChi;
      if (iter == 0) {  // computeLambdaInit (tau = 1e-5)
        double m = 0;
        for (int r = 0; r < 6; ++r) m = fmax(fabs(H[r * 6 + r]), m);
        lambda = 1e-5 * m; ni = 2; nBad = 0;
      }
      double rho = 0;
      int qmax = 0;
      do {
        const SE3 backup = T;
        double Hl[36], x[6] = {0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 36; ++k) Hl[k] = H[k];
        for (int r = 0; r < 6; ++r) Hl[r * 6 + r] += lambda;
        const bool ok2 = ldlt6(Hl, b, x);
        T = se3_mul(se3_exp(x), T);
        Teval = T;
        double tempChi = chi2Active(T);
        if (!ok2) tempChi = 1.7976931348623157e308;
        rho = currentChi - tempChi;
        double scale = 0;
        for (int r = 0; r < 6; ++r) scale += x[r] * (lambda * x[r] + b[r]);
        scale += 1e-3;
        rho /= scale;
#ifdef MORB_PO_TRACE
        if (f == 0 && tid == 0 && g_poTraceN == 0) { double* t = g_poTrace + 6 * 500; for (int k = 0; k < 6; ++k) t[k] = x[k]; for (int k = 0; k < 4; ++k) t[6 + k] = Teval.q[k]; for (int k = 0; k < 3; ++k) t[10 + k] = Teval.t[k]; }
        if (f == 0 && tid == 0 && g_poTraceN < 500) { double* t = g_poTrace + 6 * g_poTraceN++; t[0] = currentChi; t[1] = tempChi; t[2] = lambda; t[3] = rho; t[4] = scale; t[5] = ok2; }
#endif
        if (rho > 0 && isfinite(tempChi)) {
          double alpha = 1. - cube_rn(2 * rho - 1);
          alpha = fmin(alpha, 2. / 3.);
          lambda *= fmax(1. / 3., alpha);
          ni = 2;
          currentChi = tempChi;
        } else {
          lambda *= ni;
          ni *= 2;
          T = backup;
        }
        ++qmax; ++trials;
      } while (rho < 0 && qmax < 10);
      if (qmax == 10 || rho == 0) break;
      if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
      if (nBad >= 3) break;
    }
    // ---- classify (:966-1037): inlier edges keep the error of the LAST evaluated state (Teval, which is a
    // rejected trial when the LM loop ended on a failure), current outliers are re-evaluated at the final pose
    int bad = 0;
    __syncthreads();
    const SE3 TrFin = FISH ? se3_mul(rig.Trl, T) : T, TrEval = FISH ? se3_mul(rig.Trl, Teval) : Teval;
    for (int i = tid; i < n; i += NT) {
      if (!hasMP[base + i]) continue;
      const float* o = obs + (base + i) * 3;
      const double X[3] = {(double)Xw[(base + i) * 3], (double)Xw[(base + i) * 3 + 1], (double)Xw[(base + i) * 3 + 2]};
      double xc[3], err[3];
      bool st;
      const SE3& Pc = outlier[base + i] ? T : Teval;
      const float chi2 = (float)pose_edge_error<FISH>(cam, rig, Pc, outlier[base + i] ? TrFin : TrEval, FISH && i >= nL, X, o,
                                                      (double)invSigma2[base + i], err, st, xc);
      const bool isOut = chi2 > (st ? 7.815f : 5.991f);
      outlier[base + i] = isOut ? 1 : 0;
      bad += isOut ? 1 : 0;
    }
    nBadEdges = (int)block_sum_d<NW>((double)bad, red);
    if (it == 2) robust = false;
    if (nInit < 10) break;  // optimizer.edges().size() < 10 (:1039)
  }
  if (tid == 0) {
    for (int k = 0; k < 4; ++k) poseIO[7 * f + k] = (float)T.q[k];
    for (int k = 0; k < 3; ++k) poseIO[7 * f + 4 + k] = (float)T.t[k];
    nInliers[f] = nInit - nBadEdges;
    if (stats) { stats[2 * f] = outerIts; stats[2 * f + 1] = trials; }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Round 5: PoseOptimization rebuilt around what a lone frame's latency is made of (the launch is one frame's latency for 1 .. 256 frames).
//  * The active edges (map point present, not an outlier of the previous round) are COMPACTED, in feature order, at the start of each of
//    the four rounds, and every worker thread keeps its <= PO2_EPT edges in registers for the round: no global load inside the LM loop, and
//    the edge-order sums run over the active edges only (a skipped edge contributed an exact +0.0: same bits) — ~600 of 1200 features.
//  * ONE pass over the edges per LM trial instead of two.  g2o evaluates the errors twice at every accepted state: once for the trial's
//    chi2 (optimization_algorithm_levenberg.cpp:118-120) and once more, with the Jacobians, when the next iteration builds H and b
//    (:77-84).  Here the trial's pass speculatively produces H, b AND chi2 at the trial state; accepted (the common case), the next
//    iteration takes them as they are — the same expressions on the same inputs, so the same bits — and a rejected trial keeps the H, b of
//    the state it falls back to, as g2o does.
//  * In the edge-order mode wave 0 owns the 28 ordered sums and the 6 x 6 solve; waves 1 .. 7 compute the edges.  A stage is 448 edges:
//    while wave 0 adds stage s, the workers already compute stage s + 1.
//  * The solve, exp and pose update run on wave 0 only; the other waves pick the new pose up from LDS (they used to repeat all of it).
#ifndef MORB_PO2_EPT
#define MORB_PO2_EPT 4   // edges a worker thread keeps in registers per round
#endif
constexpr int PO2_NT = 512, PO2_NW = PO2_NT / 64, PO2_EPT = MORB_PO2_EPT;
// edges per stage of the edge-order mode: every wave but the summing one(s) computes edges
__host__ __device__ constexpr int po2_stage(bool mfma) { return PO2_NT - 64 * (mfma ? 2 : 1); }   // (matrix-core chain: waves 0 and 1 carry 16 + 12 sums)
// matrix-core chain: the FIRST stage is computed by all eight waves (the summing waves have nothing to add yet) and holds PO2_NT edges
__host__ __device__ constexpr int po2_rows(bool mfma) { return mfma ? PO2_NT : po2_stage(false); }   // rows of the contribution buffer
#ifndef MORB_PO2_SKIP_ROUNDS
#define MORB_PO2_SKIP_ROUNDS 1   // a round that would repeat the one before it bit for bit is not run
#endif
#ifndef MORB_PO2_SPEC
#define MORB_PO2_SPEC 1      // matrix-core chain: an iteration's first solve carries the nine trials that can follow it (one lambda per lane)
#endif
#ifndef MORB_PO2_PREVIEW
#define MORB_PO2_PREVIEW 1   // ... and a trial that follows a rejection is first judged by a tree sum of its chi2 (a rigorous "certainly rejected" test)
#endif
// frames beyond the registers' stages (PO2_NT + (PO2_EPT - 1) x stage edges) read the further edges again in every pass; the list of active features
// (two bytes per feature) has to fit in LDS beside the contribution buffer
constexpr int PO2_MAX_CAP = 8192;

struct PoEdge { float o[3], X[3], info; int right; };

// (OUT: double (&)[28] registers, or a pointer to the edge's row of the LDS buffer — the first stage writes every entry as soon as it exists, so the
// 28 x 8 bytes x 448 edges do not arrive at the LDS together at the end of the stage: the write port moves 128 bytes per cycle)
template <bool FISH, class OUT>
__device__ __forceinline__ void po2_contrib(const Cam& cam, const Rig& rig, const SE3& P, const SE3& Pr, const PoEdge& e, bool robust,
                                            double deltaMono, double deltaStereo, OUT&& con) {
  const double X[3] = {(double)e.X[0], (double)e.X[1], (double)e.X[2]};
  double xc[3], err[3], Jp[18], w = 1.0;
  bool st;
  const double info = (double)e.info;
  const bool right = FISH && e.right;
  double c = pose_edge_error<FISH>(cam, rig, P, Pr, right, X, e.o, info, err, st, xc);
  if (robust) c = huber(st ? deltaStereo : deltaMono, c, &w);
  con[27] = c;
  pose_edge_jac<FISH>(cam, rig, right, st, xc, Jp);
  // g2o's own expressions (base_unary_edge.hpp:54-66): omega_r = -Omega e (then * rho'), b += J^T omega_r, H += J^T (rho' Omega) J
  const double wr[3] = {-info * err[0] * w, -info * err[1] * w, -info * err[2] * w};
  const double wo = w * info;
  // Entries of Jp that are zero BY CONSTRUCTION are left out of the sums: pinhole (jac_pose, unary): Jp[0][4], Jp[1][3], Jp[2][4] (and a mono
  // edge's whole third row, which a stereo lane of the same wave needs); KB8: the third row.  Their products are exact zeros, x + 0 = x, and a
  // sum that starts with its first term instead of 0.0 + term differs at most in the SIGN of a zero — which the edge-order sums (they start at
  // +0.0 and can never reach -0.0) and the tree sums do not see.  63 -> 45 products for H, 18 -> 15 for b: a sixth of the edge's FP64 instructions.
  auto nz = [](int k, int r) { return FISH ? k < 2 : !((k == 0 && r == 4) || (k == 1 && r == 3) || (k == 2 && r == 4)); };
  int q = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double bb = 0;
    bool first = true;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (nz(k, r)) { const double t = Jp[k * 6 + r] * wr[k]; bb = first ? t : bb + t; first = false; }
    con[21 + r] = bb;
#pragma unroll
    for (int cc = 0; cc <= r; ++cc) {   // the LOWER triangle, (J_r w Omega) J_c as Eigen forms it: LinearSolverDense's LDLT reads that triangle
      double h = 0;
      bool firstH = true;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (nz(k, r) && nz(k, cc)) { const double t = Jp[k * 6 + r] * wo * Jp[k * 6 + cc]; h = firstH ? t : h + t; firstH = false; }
      con[q++] = h;
    }
  }
}

#ifdef MORB_PO_CYCLES   // developer build (tools/ab_build.py): thread 0 of frame 0 adds up where its cycles go
__device__ unsigned long long g_po2Cyc[8];
extern "C" int morb_po2_cycles(unsigned long long* out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_po2Cyc), sizeof(unsigned long long) * 8); const unsigned long long z[8] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_po2Cyc), z, sizeof z); return 0; }
#define PO2_T0(v) const long long v = clock64()
#define PO2_ADD(slot, v) do { if (f == 0 && tid == 0) g_po2Cyc[slot] += (unsigned long long)(clock64() - v); } while (0)
#define PO2_CNT(slot) do { if (f == 0 && tid == 0) g_po2Cyc[slot] += 1; } while (0)
#define PO2_ADD_T(slot, v, t) do { if (f == 0 && tid == (t)) g_po2Cyc[slot] += (unsigned long long)(clock64() - v); } while (0)   // (timed by thread t)
#else
#define PO2_ADD_T(slot, v, t)
#define PO2_T0(v)
#define PO2_ADD(slot, v)
#define PO2_CNT(slot)
#endif
template <bool FISH, bool ORDERED, bool MFMA, bool BIG>
__global__ __launch_bounds__(PO2_NT) void k_pose_opt2(int cap, const int* __restrict__ count, const uint8_t* __restrict__ hasMP,
                                                      const float* __restrict__ obs, const float* __restrict__ invSigma2,
                                                      const float* __restrict__ Xw, Cam cam, Rig rig, const int* __restrict__ nLeft,
                                                      float* __restrict__ poseIO, uint8_t* __restrict__ outlier,
                                                      int* __restrict__ nInliers, int* __restrict__ stats) {
  constexpr int NT = PO2_NT, NW = PO2_NW;
  constexpr int NCW = MFMA ? 2 : 1;             // waves that carry the ordered sums (wave 0 also solves)
  constexpr int W0 = ORDERED ? 64 * NCW : 0;    // first worker thread
  constexpr int NWORK = NT - W0;                // edges per stage
  static_assert(!ORDERED || NWORK == po2_stage(MFMA), "stage size");
  extern __shared__ __align__(16) uint8_t po2Raw[];
  constexpr int ROWS = po2_rows(MFMA);          // rows of the contribution buffer
  constexpr int S0 = ORDERED && MFMA ? NT : NWORK;   // edges of the first stage (matrix-core chain: every wave computes, the summing ones included)
  double* sC = reinterpret_cast<double*>(po2Raw);                                          // ORDERED: [ROWS][PO_PITCH] contributions of a stage
  uint16_t* actList = reinterpret_cast<uint16_t*>(po2Raw + (ORDERED ? (size_t)ROWS * PO_PITCH * 8 + 32 : 0));   // [cap] active features, in order

  __shared__ double red[NW];
  __shared__ double sH[NW][28];
  __shared__ double sTot[2][28];     // H (lower triangle 0 .. 20), b (21 .. 26), robust chi2 (27) at the state last built / at the trial state
  __shared__ double sKeep[3][7];     // uniform poses that would otherwise sit in every thread's registers: T0, Teval, the trial's backup
  __shared__ double sSpec[10][8];    // trial poses + scales of an iteration: slot q = its trial q (if trials 0 .. q - 1 are rejected)
  __shared__ int sSpecFlag[10];
  __shared__ double sChiA[2][NW];    // the waves' partial sums of a trial's chi2 preview, by trial parity
  __shared__ int sWaveCnt[NW];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = min(count ? count[f] : cap, cap);
  const size_t base = (size_t)f * cap;
  const double deltaMono = (double)(float)sqrt(5.991), deltaStereo = (double)(float)sqrt(7.815);
  // this thread's row in a stage (-1: not a worker)
  const int wrow = tid >= W0 ? tid - W0 : -1;
  // Speculation (matrix-core chain): a rejected trial is followed by a trial from the SAME state with lambda * ni, the next one with that * 2 ni, ... —
  // everything the solves of an iteration's up to ten trials need is known when its first trial is solved.  Wave 0's solve is uniform code, so its
  // lanes carry all ten at once: lane g the trial with lambda_g (the bookkeeping's own `lambda *= ni; ni *= 2`, g times: the same bits).  The ~5 k
  // cycles of LDL^T + exp + pose update are paid once per iteration instead of once per trial (more than half of all trials follow a rejection: near
  // convergence g2o's LM rejects its way up in lambda, up to ten trials per iteration).
  const bool spec = ORDERED && MFMA && MORB_PO2_SPEC;
  const int s0 = S0, nwork = NWORK;   // edges of the first / of a later stage
  // the edge thread `tid` computes in stage s (its row of the stage, the stage's first edge)
  auto stage_row = [&](int s) { return ORDERED && (s > 0 || !MFMA) ? (wrow < nwork ? wrow : -1) : (tid < s0 ? tid : -1); };
  auto stage_base = [&](int s) { return s == 0 ? 0 : s0 + (s - 1) * nwork; };

  PO2_T0(tAll);
#ifdef MORB_PO_FRAME_CYCLES
  const long long tFrame0 = clock64();
  int nCertain = 0;
#endif
  int nInit = 0;
  for (int i = tid; i < n; i += NT) {
    if (hasMP[base + i]) { ++nInit; outlier[base + i] = 0; }
  }
  nInit = (int)block_sum_d<NW>((double)nInit, red);
  if (nInit < 3) {  // Optimizer.cc:951
    if (tid == 0) { nInliers[f] = 0; if (stats) { stats[2 * f] = 0; stats[2 * f + 1] = 0; } }
    return;
  }
  SE3 T = se3_from_float(poseIO + 7 * f);
  auto put = [&](int slot, const SE3& P) { if (tid == 0) { for (int k = 0; k < 4; ++k) sKeep[slot][k] = P.q[k]; for (int k = 0; k < 3; ++k) sKeep[slot][4 + k] = P.t[k]; } };
  auto get = [&](int slot) { SE3 P; for (int k = 0; k < 4; ++k) P.q[k] = sKeep[slot][k]; for (int k = 0; k < 3; ++k) P.t[k] = sKeep[slot][4 + k]; return P; };
  put(0, T); put(1, T);     // T0, Teval (read after later barriers)
  bool robust = true;
  int nBadEdges = 0, outerIts = 0, trials = 0;
  const int nL = FISH ? nLeft[f] : n;   // features >= nL are right-camera observations (fisheye rig)
  PoEdge ed[PO2_EPT];
  int nAct = 0;
  bool sawReject = false;   // first trials are previewed once a trial of this call was rejected (measured best: 318 k frames/s against 312 k per round, 317 k always)

  auto load_edge = [&](int i, PoEdge& e) {
    e.o[0] = obs[(base + i) * 3]; e.o[1] = obs[(base + i) * 3 + 1]; e.o[2] = obs[(base + i) * 3 + 2];
    e.X[0] = Xw[(base + i) * 3]; e.X[1] = Xw[(base + i) * 3 + 1]; e.X[2] = Xw[(base + i) * 3 + 2];
    e.info = invSigma2[base + i];
    e.right = i >= nL;
  };
  // The solve of an iteration's trials, by wave 0: (H + lam I) x = b of sTot[src], Tn = exp(x) Tb, scale = x . (lam x + b) + 1e-3.  Lane g < nTrials solves
  // trial g — lam_g = lam after g rejections — and writes sSpec[g] / sSpecFlag[g]; the other lanes repeat lane nTrials - 1's arithmetic.
  auto solve_trials = [&](int src, double lam, double niv, const SE3& Tb, int nTrials) {
    const int g = min(lane, nTrials - 1);
    for (int j = 0; j < g; ++j) { lam *= niv; niv *= 2; }
    double H[36], b[6], x[6];
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int cc = 0; cc <= r; ++cc) { const double v = sTot[src][q++]; H[r * 6 + cc] = v; H[cc * 6 + r] = v; }
#pragma unroll
    for (int r = 0; r < 6; ++r) { b[r] = sTot[src][21 + r]; H[r * 6 + r] += lam; x[r] = 0; }
    const bool ok2 = ldlt6(H, b, x);
    const SE3 Tn = se3_mul(se3_exp(x), Tb);
    double scale = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) scale += x[r] * (lam * x[r] + b[r]);
    scale += 1e-3;
    if (lane < nTrials) {
      double* o8 = sSpec[lane];
      for (int k = 0; k < 4; ++k) o8[k] = Tn.q[k];
      for (int k = 0; k < 3; ++k) o8[4 + k] = Tn.t[k];
      o8[7] = scale;
      sSpecFlag[lane] = ok2 ? 1 : 0;
    }
  };
  // H, b, chi2 of the active edges at pose P -> sTot[buf]
  auto pass = [&](const SE3& P, int buf) {
    PO2_T0(tp); PO2_CNT(4);
    const SE3 Pr = FISH ? se3_mul(rig.Trl, P) : P;
    if (ORDERED) {
      double tot = 0;   // VALU chain: lanes 0 .. 27 of wave 0 hold entry `lane`; matrix-core chain: the accumulator (D layout) of waves 0 and 1
      const int nAct16 = (nAct + 15) & ~15;
#pragma unroll
      for (int s = 0; s < PO2_EPT; ++s) {   // (unrolled: ed[s] must stay in registers)
        const int e0 = stage_base(s), row = stage_row(s);
        if (e0 >= nAct) break;
        double con[28];
        const int e = e0 + row;
        const bool mine = row >= 0 && e < nAct;
        // (The first stage needs no barrier in front of its LDS writes — the previous pass ended with one — and writes from inside the edge math.
        // KB8 rig: through registers in every stage — writing from inside its longer edge math costs that kernel 400 bytes of scratch memory.)
        if (mine) {
          if (s == 0 && !FISH) po2_contrib<FISH>(cam, rig, P, Pr, ed[s], robust, deltaMono, deltaStereo, sC + row * PO_PITCH);
          else po2_contrib<FISH>(cam, rig, P, Pr, ed[s], robust, deltaMono, deltaStereo, con);   // (beside the sums of stage s - 1)
        }
        if (s == 0) PO2_ADD_T(3, tp, NT - 64);   // (a worker's edge math of the first stage)
        // Stage s - 1 has been added.  (Measured and not kept: progress words published by the summing waves, so that a later stage's writers wait for
        // their own row instead of this barrier — 0.404 -> 0.435 ms per launch: writes that arrive while the sums run delay the sums' LDS reads.)
        if (s > 0) __syncthreads();
        if (mine && (s > 0 || FISH)) {
#pragma unroll
          for (int k = 0; k < 28; ++k) sC[row * PO_PITCH + k] = con[k];
        } else if (!mine && MFMA && row >= 0 && e < nAct16) {   // the matrix core takes four rows at a time: the last batch's missing rows add 0.0
#pragma unroll
          for (int k = 0; k < 28; ++k) sC[row * PO_PITCH + k] = 0.0;
        }
        __syncthreads();
        PO2_T0(tch);
        const int m = min(s == 0 ? s0 : nwork, (MFMA ? nAct16 : nAct) - e0);
        if (MFMA) { if (wv < 2) ordered_add_mfma1<PO_PITCH, ROWS>(tot, sC + 16 * wv, lane, m); }
        else if (tid < 28) tot = ordered_add_pipe<PO_PITCH, ROWS>(tot, sC + tid, m);
        PO2_ADD(7, tch);
      }
      // frames with more active edges than the threads' registers hold (PO2_EPT stages): the further stages read their edge again in every pass
      if (BIG) for (int s = PO2_EPT; stage_base(s) < nAct; ++s) {
        const int e0 = stage_base(s), row = stage_row(s);
        double con[28];
        const int e = e0 + row;
        const bool mine = row >= 0 && e < nAct;
        if (mine) {
          PoEdge ee;
          load_edge(actList[e], ee);
          po2_contrib<FISH>(cam, rig, P, Pr, ee, robust, deltaMono, deltaStereo, con);
        }
        __syncthreads();
        if (mine) {
#pragma unroll
          for (int k = 0; k < 28; ++k) sC[row * PO_PITCH + k] = con[k];
        } else if (MFMA && row >= 0 && e < nAct16) {
#pragma unroll
          for (int k = 0; k < 28; ++k) sC[row * PO_PITCH + k] = 0.0;
        }
        __syncthreads();
        const int m = min(nwork, (MFMA ? nAct16 : nAct) - e0);
        if (MFMA) { if (wv < 2) ordered_add_mfma1<PO_PITCH, ROWS>(tot, sC + 16 * wv, lane, m); }
        else if (tid < 28) tot = ordered_add_pipe<PO_PITCH, ROWS>(tot, sC + tid, m);
      }
      if (MFMA) {
        const int c16 = 4 * ((lane >> 2) & 3) + (lane >> 4);
        if (wv < 2 && (lane & 3) == 0 && 16 * wv + c16 < 28) sTot[buf][16 * wv + c16] = tot;
      } else if (tid < 28) sTot[buf][tid] = tot;
      __syncthreads();
      PO2_ADD(2, tp);
    } else {
      double acc[28];
#pragma unroll
      for (int k = 0; k < 28; ++k) acc[k] = 0;
#pragma unroll
      for (int s = 0; s < PO2_EPT; ++s) {
        if (s * NWORK + tid < nAct) {
          double con[28];
          po2_contrib<FISH>(cam, rig, P, Pr, ed[s], robust, deltaMono, deltaStereo, con);
#pragma unroll
          for (int k = 0; k < 28; ++k) acc[k] += con[k];
        }
      }
      if (BIG) for (int e = PO2_EPT * NWORK + tid; e < nAct; e += NWORK) {   // (larger frames: the edge is read again in every pass)
        PoEdge ee;
        load_edge(actList[e], ee);
        double con[28];
        po2_contrib<FISH>(cam, rig, P, Pr, ee, robust, deltaMono, deltaStereo, con);
#pragma unroll
        for (int k = 0; k < 28; ++k) acc[k] += con[k];
      }
      __syncthreads();                         // (sH / sTot[buf] of an earlier pass have been read)
      wave_sum28_to(acc, sH[wv], lane);
      __syncthreads();
      if (tid < 28) { double t = sH[0][tid]; for (int w = 1; w < NW; ++w) t += sH[w][tid]; sTot[buf][tid] = t; }
      __syncthreads();
      PO2_ADD(2, tp);
    }
  };

  // A round whose classification changes no flag is followed by an IDENTICAL round (same active edges, same start pose, same robust kernel: rounds 1 - 3 of
  // the reference's four all use the Huber kernel; the computation is deterministic) that would end in the same pose and the same flags: it is not run,
  // its iterations and trials are counted.  (Outlier sets usually settle after the first round or two; the fourth round, without the kernel, always runs.)
  // (decided at the END of a round — the loop counter jumps over the rounds that would repeat it: no second path around the round's body)
  for (int it = 0; it < 4; ++it) {
    const int its0 = outerIts, trials0 = trials;
    // ---- the round's active edges, in feature order; each worker thread takes its edges into registers
    PO2_T0(tc);
    __syncthreads();
    T = get(0);  // vSE3->setEstimate(pFrame->GetPose()) (:962-964)
    nAct = 0;
    for (int c0 = 0; c0 < n; c0 += NT) {
      const int i = c0 + tid;
      const bool a = i < n && hasMP[base + i] && !outlier[base + i];
      const unsigned long long m = __ballot(a);
      if (lane == 0) sWaveCnt[wv] = __popcll(m);
      __syncthreads();
      int off = nAct, totc = 0;
      for (int w = 0; w < NW; ++w) { const int c = sWaveCnt[w]; if (w < wv) off += c; totc += c; }
      if (a) actList[off + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)i;
      nAct += totc;
      __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < PO2_EPT; ++s) {
      const int e = stage_base(s) + stage_row(s);
      if (stage_row(s) >= 0 && e < nAct) {
        load_edge(actList[e], ed[s]);
      }
    }
    PO2_ADD(5, tc);
    // ---- optimizer.optimize(10) ----
    int cur = 0;
    pass(T, cur);
    double lambda = 0, ni = 2;
    int nBad = 0;
    for (int iter = 0; iter < 10; ++iter) {
      ++outerIts;
      double currentChi = sTot[cur][27];
      const double iniChi = currentChi;
      if (iter == 0) {  // computeLambdaInit (tau = 1e-5)
        double m = 0;
        int q = 0;
        for (int r = 0; r < 6; ++r) { q += r; m = fmax(fabs(sTot[cur][q + r]), m); }   // diagonal entries of the packed lower triangle
        lambda = 1e-5 * m; ni = 2; nBad = 0;
      }
      double rho = 0;
      int qmax = 0;
      do {
        PO2_T0(ts);
        // the iteration's first trial (every trial without the speculation): the solve; a trial after a rejection finds its pose in its slot
        if (qmax == 0 || !spec) {
          if (qmax == 0) put(2, T);           // backup (thread 0 writes it, its own wave reads it back below: LDS operations of a wave execute in order)
          if (wv == 0) solve_trials(cur, lambda, ni, get(2), spec ? 10 : 1);   // (the slots' last readers are behind the barriers of the pass before)
          __syncthreads();
        }
        const int sl = spec ? qmax : 0;
        for (int k = 0; k < 4; ++k) T.q[k] = sSpec[sl][k];
        for (int k = 0; k < 3; ++k) T.t[k] = sSpec[sl][4 + k];
        const double scale = sSpec[sl][7];
        const bool ok2 = sSpecFlag[sl] != 0;
        PO2_ADD(1, ts);
        put(1, T);           // Teval
        // A trial that follows a rejection is usually rejected too (g2o's LM climbs in lambda near convergence), and a rejected trial leaves nothing
        // behind but the decision rho <= 0: its H, b and even its chi2 are dropped.  The decision is chi2(trial) > chi2(current state) — sums of
        // non-negative terms — so a PREVIEW decides most of them rigorously: every thread adds the robustified chi2 of its own edges (errors only: a
        // third of the edge math), a tree sum over the workgroup, and since two floating-point sums of the same n non-negative terms differ by less
        // than 2 n 2^-53 of their value (any order, any association), `preview (1 - 8 n 2^-53) > currentChi` implies that the edge-order sum is larger
        // too: rejected, for certain, without the edge-order sums, the Jacobians or the LDS hand-over (measured on the oracle's traces: 90 % of the
        // rejections, half of all trials).  Otherwise the trial runs its pass as before.  (Its pose has been waiting since the iteration's first trial.)
        bool certainlyRejected = false;
        if (spec && MORB_PO2_PREVIEW && (qmax > 0 || sawReject) && ok2 && scale > 0) {   // (an iteration's first trial too once this call has rejected one)
          const int par = trials & 1;
          double part = 0;
          {
            const SE3 Tr = FISH ? se3_mul(rig.Trl, T) : T;
#pragma unroll
            for (int s = 0; s < PO2_EPT; ++s) {
              const int row = stage_row(s), e = stage_base(s) + row;
              if (row >= 0 && e < nAct) {
                const double X[3] = {(double)ed[s].X[0], (double)ed[s].X[1], (double)ed[s].X[2]};
                double xc[3], err[3], w;
                bool st;
                double c = pose_edge_error<FISH>(cam, rig, T, Tr, FISH && ed[s].right, X, ed[s].o, (double)ed[s].info, err, st, xc);
                if (robust) c = huber(st ? deltaStereo : deltaMono, c, &w);
                part += c;
              }
            }
          }
          if (BIG) {
            const SE3 Tr = FISH ? se3_mul(rig.Trl, T) : T;
            for (int s = PO2_EPT; stage_base(s) < nAct; ++s) {   // (the stages whose edges are not in registers)
              const int row = stage_row(s), e = stage_base(s) + row;
              if (row >= 0 && e < nAct) {
                PoEdge ee;
                load_edge(actList[e], ee);
                const double X[3] = {(double)ee.X[0], (double)ee.X[1], (double)ee.X[2]};
                double xc[3], err[3], w;
                bool st;
                double c = pose_edge_error<FISH>(cam, rig, T, Tr, FISH && ee.right, X, ee.o, (double)ee.info, err, st, xc);
                if (robust) c = huber(st ? deltaStereo : deltaMono, c, &w);
                part += c;
              }
            }
          }
          part = wave_sum_d(part);
          if (lane == 0) sChiA[par][wv] = part;
          __syncthreads();
          double tt = 0;
#pragma unroll
          for (int w = 0; w < NW; ++w) tt += sChiA[par][w];
          certainlyRejected = isfinite(tt) && tt * (1.0 - 8.0 * (double)nAct * 0x1p-53) > currentChi;
        }
        double tempChi = 1.7976931348623157e308;
        if (!certainlyRejected) {
          pass(T, cur ^ 1);
          tempChi = sTot[cur ^ 1][27];
          if (!ok2) tempChi = 1.7976931348623157e308;
        }
#ifdef MORB_PO_FRAME_CYCLES
        nCertain += certainlyRejected ? 1 : 0;
#endif
        rho = certainlyRejected ? -1.0 : (currentChi - tempChi) / scale;   // (a certainly rejected trial: only the sign of rho is ever read)
        if (rho > 0 && isfinite(tempChi)) {
          double alpha = 1. - cube_rn(2 * rho - 1);
          alpha = fmin(alpha, 2. / 3.);
          lambda *= fmax(1. / 3., alpha);
          ni = 2;
          currentChi = tempChi;
          cur ^= 1;           // H, b at the accepted state are already there
        } else {
          lambda *= ni;
          ni *= 2;
          T = get(2);         // sTot[cur] still holds H, b of this state
          sawReject = true;
        }
        ++qmax; ++trials;
      } while (rho < 0 && qmax < 10);
      if (qmax == 10 || rho == 0) break;
      if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
      if (nBad >= 3) break;
    }
    // ---- classify (:966-1037): inlier edges keep the error of the LAST evaluated state (Teval, which is a
    // rejected trial when the LM loop ended on a failure), current outliers are re-evaluated at the final pose
    int bad = 0;
    PO2_T0(tk);
    __syncthreads();
    const SE3 Teval = get(1);
    const SE3 TrFin = FISH ? se3_mul(rig.Trl, T) : T, TrEval = FISH ? se3_mul(rig.Trl, Teval) : Teval;
    for (int i = tid; i < n; i += NT) {
      if (!hasMP[base + i]) continue;
      const float* o = obs + (base + i) * 3;
      const double X[3] = {(double)Xw[(base + i) * 3], (double)Xw[(base + i) * 3 + 1], (double)Xw[(base + i) * 3 + 2]};
      double xc[3], err[3];
      bool st;
      const bool wasOut = outlier[base + i] != 0;
      const SE3& Pc = wasOut ? T : Teval;
      const float chi2 = (float)pose_edge_error<FISH>(cam, rig, Pc, wasOut ? TrFin : TrEval, FISH && i >= nL, X, o,
                                                      (double)invSigma2[base + i], err, st, xc);
      const bool isOut = chi2 > (st ? 7.815f : 5.991f);
      outlier[base + i] = isOut ? 1 : 0;
      bad += (isOut ? 1 : 0) + (isOut != wasOut ? 65536 : 0);   // (outliers | flags that changed: two counts in one exact sum)
    }
    {
      const int packed = (int)block_sum_d<NW>((double)bad, red);
      nBadEdges = packed & 0xFFFF;
      if (MORB_PO2_SKIP_ROUNDS && (packed >> 16) == 0 && it < 2 && nInit >= 10) {   // rounds it + 1 .. 2 would repeat this one (fewer than 10 edges: one round only, :1039)
        const int k = 2 - it;
        outerIts += k * (outerIts - its0); trials += k * (trials - trials0);
        it = 2;
      }
    }
    PO2_ADD(6, tk);
    if (it == 2) robust = false;
    if (nInit < 10) break;  // optimizer.edges().size() < 10 (:1039)
  }
  if (tid == 0) {
    for (int k = 0; k < 4; ++k) poseIO[7 * f + k] = (float)T.q[k];
    for (int k = 0; k < 3; ++k) poseIO[7 * f + 4 + k] = (float)T.t[k];
    nInliers[f] = nInit - nBadEdges;
#ifdef MORB_PO_FRAME_CYCLES   // developer build: the frame's kernel time (kilocycles) and its certain rejections instead of iterations / trials
    if (stats) { stats[2 * f] = (int)((clock64() - tFrame0) / 1000); stats[2 * f + 1] = trials * 100 + nCertain; }
#else
    if (stats) { stats[2 * f] = outerIts; stats[2 * f + 1] = trials; }
#endif
  }
  PO2_ADD(0, tAll);
}
// registers hold the edges of PO2_EPT stages; larger frames run the BIG instantiation (further stages read their edge again in every pass: kept out of
// the common kernels, where the extra code costs registers — 3 % on the tracking chain)
__host__ __device__ constexpr int po2_reg_cap(bool ordered, bool mfma) {
  return !ordered ? PO2_EPT * PO2_NT : mfma ? PO2_NT + (PO2_EPT - 1) * po2_stage(true) : PO2_EPT * po2_stage(false);
}
template <bool FISH, bool ORDERED, bool MFMA, bool BIG>
static int launch_pose_opt2_as(int nframes, hipStream_t st, size_t lds, int cap, const int* d_count, const uint8_t* d_hasMP, const float* d_obs,
                               const float* d_invSigma2, const float* d_Xw, const Cam& cam, const Rig& rig, const int* d_nLeft, float* d_pose,
                               uint8_t* d_outlier, int* d_nInliers, int* d_stats) {
  if (lds > 48 * 1024)
    MORB_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pose_opt2<FISH, ORDERED, MFMA, BIG>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_pose_opt2<FISH, ORDERED, MFMA, BIG>), dim3(nframes), dim3(PO2_NT), lds, st, cap, d_count, d_hasMP, d_obs, d_invSigma2, d_Xw, cam, rig,
                     d_nLeft, d_pose, d_outlier, d_nInliers, d_stats);
  return MORB_OK;
}
// false: this mode / size has no k_pose_opt2 form (the caller launches k_pose_opt)
static bool pose_opt2_covers(bool ordered, bool mfmaChain, int cap) {
  return cap <= PO2_MAX_CAP && (cap <= po2_reg_cap(ordered, mfmaChain) || !ordered || mfmaChain);   // (no BIG form of the vector-chain mode)
}
template <bool FISH>
static int launch_pose_opt2(bool ordered, bool mfmaChain, int nframes, hipStream_t st, int cap, const int* d_count, const uint8_t* d_hasMP, const float* d_obs,
                            const float* d_invSigma2, const float* d_Xw, const Cam& cam, const Rig& rig, const int* d_nLeft, float* d_pose,
                            uint8_t* d_outlier, int* d_nInliers, int* d_stats) {
  const size_t listBytes = ((size_t)cap * 2 + 15) & ~(size_t)15;
  const bool big = cap > po2_reg_cap(ordered, mfmaChain);
  const size_t lds = ordered ? (size_t)po2_rows(mfmaChain) * PO_PITCH * 8 + 32 + listBytes : listBytes;   // (+32: the second accumulator's lanes 12 .. 15 read past the last row)
#define MORB_PO2_GO(O, M, B) return launch_pose_opt2_as<FISH, O, M, B>(nframes, st, lds, cap, d_count, d_hasMP, d_obs, d_invSigma2, d_Xw, cam, rig, d_nLeft, d_pose, d_outlier, d_nInliers, d_stats)
  if (ordered && mfmaChain) { if (big) MORB_PO2_GO(true, true, true); else MORB_PO2_GO(true, true, false); }
  if (ordered) MORB_PO2_GO(true, false, false);
  if (big) MORB_PO2_GO(false, false, true);
  MORB_PO2_GO(false, false, false);
#undef MORB_PO2_GO
}

}  // namespace

// PoseOptimization's dispatch: k_pose_opt2 where it has a form of this mode and size and the caller allows it, else k_pose_opt
template <bool FISH>
static int pose_optimization(const morb_optimizer* o, bool allowOpt2, int nframes, hipStream_t st, int cap, const int* d_count, const uint8_t* d_hasMP,
                             const float* d_obs, const float* d_invSigma2, const float* d_Xw, const Cam& cam, const Rig& rig, const int* d_nLeft,
                             float* d_pose, uint8_t* d_outlier, int* d_nInliers, int* d_stats) {
  if (pose_opt2_covers(o->exactOrder != 0, o->mfmaChain != 0, cap) && allowOpt2) {
    const int rc = launch_pose_opt2<FISH>(o->exactOrder != 0, o->mfmaChain != 0, nframes, st, cap, d_count, d_hasMP, d_obs, d_invSigma2, d_Xw, cam, rig, d_nLeft, d_pose,
                                          d_outlier, d_nInliers, d_stats);
    if (rc != MORB_OK) return rc;
  } else if (o->exactOrder) {
    hipLaunchKernelGGL((k_pose_opt<FISH, true, 256>), dim3(nframes), dim3(256), 0, st, cap, d_count, d_hasMP, d_obs, d_invSigma2, d_Xw, cam, rig,
                       d_nLeft, d_pose, d_outlier, d_nInliers, d_stats);
  } else {
    hipLaunchKernelGGL((k_pose_opt<FISH, false, MORB_PO_NT>), dim3(nframes), dim3(MORB_PO_NT), 0, st, cap, d_count, d_hasMP, d_obs, d_invSigma2, d_Xw, cam, rig,
                       d_nLeft, d_pose, d_outlier, d_nInliers, d_stats);
  }
  MORB_HIP_CHECK(hipGetLastError());
  return MORB_OK;
}

extern "C" {

int morb_optimizer_create(morb_optimizer** out, int device) {
  MORB_REQUIRE(out, MORB_ERR_INVALID, "out is NULL");
  *out = nullptr;
  int ndev = 0;
  MORB_HIP_CHECK(hipGetDeviceCount(&ndev));
  MORB_REQUIRE(device >= 0 && device < ndev, MORB_ERR_INVALID, "no such HIP device");
  MORB_HIP_CHECK(hipSetDevice(device));
  std::unique_ptr<morb_optimizer> o(new morb_optimizer());
  o->device = device;
  if (o->stream.create(hipStreamDefault) != hipSuccess || o->side.create(hipStreamNonBlocking) != hipSuccess ||
      o->evFork.create(hipEventDisableTiming) != hipSuccess || o->evJoin.create(hipEventDisableTiming) != hipSuccess) {
    set_error("cannot create stream");
    return MORB_ERR_HIP;
  }
  {  // may the matrix core carry the edge-order sums?  (one 64-thread launch per handle; MORB_PO2_CHAIN = valu | mfma overrides)
    const char* force = getenv("MORB_PO2_CHAIN");
    if (force && (!strcmp(force, "valu") || !strcmp(force, "mfma"))) o->mfmaChain = force[0] == 'm';
    else {
      morb::DeviceArray<int> d_bad;
      int bad = -1;
      if (d_bad.alloc(sizeof(int)) == hipSuccess && hipMemsetAsync(d_bad, 0, sizeof(int), o->stream) == hipSuccess) {
        hipLaunchKernelGGL(k_mfma_order_selftest, dim3(1), dim3(64), 0, o->stream, 1024, d_bad.get());
        if (hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, o->stream) != hipSuccess || hipStreamSynchronize(o->stream) != hipSuccess) bad = -1;
      }
      o->mfmaChain = bad == 0;
      o->mfmaSelftest = bad < 0 ? -1 : (bad == 0 ? 1 : 0);
    }
  }
  *out = o.release();
  return MORB_OK;
}

void* morb_optimizer_stream(const morb_optimizer* o) { return o ? (void*)o->stream : nullptr; }
int morb_optimizer_lm_words(morb_optimizer* o, int** host, int** dev) {
  MORB_REQUIRE(o && host && dev, MORB_ERR_INVALID, "NULL argument");
  if (!o->lmWords) {
    MORB_HIP_CHECK(o->lmWords.alloc(sizeof(int) * 16, hipHostMallocMapped));
    memset(o->lmWords, 0, sizeof(int) * 16);
  }
  *host = o->lmWords; *dev = o->lmWords.dev();
  return MORB_OK;
}

int morb_optimizer_info(const morb_optimizer* o, int* mfma_chain, int* exact_order, int* mfma_selftest) {
  MORB_REQUIRE(o, MORB_ERR_INVALID, "NULL optimizer");
  if (mfma_chain) *mfma_chain = o->mfmaChain;
  if (exact_order) *exact_order = o->exactOrder;
  if (mfma_selftest) *mfma_selftest = o->mfmaSelftest;
  return MORB_OK;
}

int morb_optimizer_set_exact_order(morb_optimizer* o, int on) {
  MORB_REQUIRE(o, MORB_ERR_INVALID, "NULL optimizer");
  o->exactOrder = on ? 1 : 0;
  return MORB_OK;
}

int morb_optimizer_sync(morb_optimizer* o) {
  MORB_REQUIRE(o, MORB_ERR_INVALID, "NULL optimizer");
  MORB_HIP_CHECK(hipSetDevice(o->device));
  MORB_HIP_CHECK(hipStreamSynchronize(o->stream));
  return MORB_OK;
}

void morb_optimizer_destroy(morb_optimizer* o) {
  if (!o) return;
  (void)hipSetDevice(o->device);
  (void)hipStreamSynchronize(o->stream);
  (void)hipStreamSynchronize(o->side);
  delete o;
}

int morb_pose_optimization_batch(morb_optimizer* o, int nframes, int cap, const int* d_count, const uint8_t* d_hasMP,
                                 const float* d_obs, const float* d_invSigma2, const float* d_Xw, float fx, float fy,
                                 float cx, float cy, float bf, float* d_pose, uint8_t* d_outlier, int* d_nInliers,
                                 int* d_stats, void* stream) {
  MORB_REQUIRE(o && d_hasMP && d_obs && d_invSigma2 && d_Xw && d_pose && d_outlier && d_nInliers, MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nframes > 0 && cap > 0, MORB_ERR_INVALID, "bad sizes");
  MORB_ENTER(st, o, stream);
  Cam cam{fx, fy, cx, cy, bf};
  Rig rig;
  memset(&rig, 0, sizeof rig);
  // (tree-sum mode on small frames: k_pose_opt2's 512 threads take ONE edge each, so a frame with 513 .. 640 active edges pays a second, nearly
  // empty stage per pass — 0.447 against 0.400 ms per launch at 600 features; k_pose_opt's 256 threads with 2 - 3 edges each stay the faster
  // form there.  Frames of ~1200 features of which half hold a map point — tracking — are where the compaction of k_pose_opt2 pays.)
  const bool smallTree = !o->exactOrder && cap <= 640;
  return pose_optimization<false>(o, !smallTree, nframes, st, cap, d_count, d_hasMP, d_obs, d_invSigma2, d_Xw, cam, rig, nullptr, d_pose, d_outlier,
                                  d_nInliers, d_stats);
}

int morb_pose_optimization_fisheye_batch(morb_optimizer* o, int nframes, int cap, const int* d_count, const int* d_nLeft,
                                         const uint8_t* d_hasMP, const float* d_obs, const float* d_invSigma2,
                                         const float* d_Xw, const float* camL8, const float* camR8, const float* Trl7,
                                         float* d_pose, uint8_t* d_outlier, int* d_nInliers, int* d_stats, void* stream) {
  MORB_REQUIRE(o && d_count && d_nLeft && d_hasMP && d_obs && d_invSigma2 && d_Xw && camL8 && camR8 && Trl7 && d_pose && d_outlier &&
                   d_nInliers, MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nframes > 0 && cap > 0, MORB_ERR_INVALID, "bad sizes");
  MORB_ENTER(st, o, stream);
  Cam cam{0, 0, 0, 0, 0};
  const Rig rig = make_rig(camL8, camR8, Trl7);
  return pose_optimization<true>(o, true, nframes, st, cap, d_count, d_hasMP, d_obs, d_invSigma2, d_Xw, cam, rig, d_nLeft, d_pose, d_outlier,
                                 d_nInliers, d_stats);
}

}  // extern "C"
