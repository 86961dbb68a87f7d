// Optimizer::InertialOptimization in its three overloads (reference src/Optimizer.cc:2979-3156, :3158-3314, :3316-3428; the steps behind
// LocalMapping::InitializeIMU / ScaleRefinement and the bias re-estimation of a map merge) for MI355X (gfx950), batched:
//   k_inertial_optimization — one workgroup per problem, the whole Levenberg-Marquardt (modes 0, 1) or Gauss-Newton (mode 2) run in ONE launch.
// Unknowns: one velocity per keyframe, coupled to its temporal neighbours only, and nine global ones (gyro bias 3, accelerometer bias 3,
// gravity direction 2, scale 1) coupled to everything: an arrowhead, solved as such with the steps of include/morb/arrowhead_math.h —
// cost linear in the keyframe count.  Poses are fixed.  FP64 throughout; the preintegrated deltas pass through float like the reference's.
//   * one thread per link: EdgeInertialGS error and Jacobian (G2oTypes.cc:587-727), its 15 x 15 block of J^T Omega J.  The velocity-2 rows go
//     to the link's own keyframe, the velocity-1 rows and the global block to the link's scratch record; the keyframe's thread then adds its
//     successor's velocity-1 rows, and the global block is summed IN LINK ORDER (four slices, one per wave, added in slice order): no atomics;
//   * wave 0, lanes 0..9: block LDL^T down the chain, one carried column (nine border columns, the right-hand side) per lane;
//   * all threads: the Schur sum in keyframe order per wave slice; one thread: the 9 x 9 corner; one thread: back up the chain.
// Fixed unknowns (bFixedVel, stereo's scale, modes 1 and 2) get zero Jacobian columns and a unit diagonal: they leave the solve as exact zeros.
// Per-keyframe chain storage (IO_KS doubles) lives in LDS up to IO_LDS_KF keyframes, else in the handle's global workspace; the per-link
// information matrix (9 x 9) and scratch record are always global.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "common.h"
#include "handles.h"
#include "inertial_device.h"
#include "libm_f64.h"
#include "lm_control.h"
#include "morb/arrowhead_math.h"
#include "wave.h"

using namespace morb;

#define IO_WAVE_SYNC()                                      \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); \
    __builtin_amdgcn_wave_barrier();                       \
  } while (0)

namespace {

constexpr int IO_T = 256, IO_W = IO_T / 64;
constexpr int IO_MAX_KF = 4096;
constexpr int IO_LDS_KF = 192;      // the chain of a problem stays in LDS up to this cap: 192 * IO_KS * 8 B = 149 KB beside ~9 KB of static LDS
// per-keyframe chain record (doubles): T 9 | O 9 | F = [B | r] 30 | Dinv 9 | Fp 30 | v 3 | v backup 3 | x 3; the odd stride spreads consecutive
// records over the LDS banks
constexpr int IO_T0 = 0, IO_O = 9, IO_F = 18, IO_DINV = 48, IO_FP = 57, IO_V = 87, IO_VBK = 90, IO_X = 93, IO_KS = 97;
// per-link global record (doubles): information 81 | scratch 324 (the eigenvalue clamp's workspace at set-up, then: velocity-1 rows T1 9, B1 27, r1 3,
// and the global block: upper triangle 45, right-hand side 9)
constexpr int IO_INFO = 0, IO_SCR = 81, IO_H1 = IO_SCR, IO_HG = IO_SCR + 39, IO_LS = 405;
constexpr int IO_NC = 15;           // link columns: velocity 2 (0..2), velocity 1 (3..5), gyro bias, acc bias, gravity direction (12, 13), scale (14)

struct IoGlobal { double Rwg[9], s, bg[3], ba[3]; };

struct IoShared {
  IoGlobal G, Gbk;
  double C[81], rg[9], S[81], rhs[9], g[9];
  double part[IO_W][56];
  double gj[IO_W][9 * 18];   // set-up: a link's Gauss-Jordan tile per wave
  double red[IO_W];
  int flag, nlink;
};

// EdgeInertialGS::computeError between keyframes 1 and 2 (state rows of d_kfState21; velocities and the global unknowns from the solver)
struct IoLinkGeom { double Rbw1[9], eR[9], dbg[3], dv[3], dpv[3]; };
__device__ __forceinline__ void io_link_error(const morb_imu_preintegrated& P, const float* s1, const float* s2, const double* v1, const double* v2,
                                           const IoGlobal& G, double* err, IoLinkGeom* geom) {
  double dR[9], dV[3], dP[3], dbg[3];
  imu_delta(P, G.bg, G.ba, dR, dV, dP, dbg);
  const double dt = P.dT;
  double Rwb1[9], Rwb2[9], Rbw1[9], dRt[9], M[9], eR[9], er[3];
  for (int k = 0; k < 9; ++k) { Rwb1[k] = s1[k]; Rwb2[k] = s2[k]; }
  transpose33(Rwb1, Rbw1);
  transpose33(dR, dRt);
  mul33(dRt, Rbw1, M);
  mul33(M, Rwb2, eR);
  log_so3(eR, er);
  const double G0 = (double)9.81f;
  const double g[3] = {G.Rwg[2] * -G0, G.Rwg[5] * -G0, G.Rwg[8] * -G0};   // Rwg * (0, 0, -GRAVITY_VALUE)
  double dv[3], dpv[3], t[3], a1[3], a2[3];
  for (int k = 0; k < 3; ++k) {
    dv[k] = v2[k] - v1[k];
    dpv[k] = (double)s2[9 + k] - (double)s1[9 + k] - v1[k] * dt;
  }
  for (int k = 0; k < 3; ++k) t[k] = G.s * dv[k] - g[k] * dt;
  mul3v(Rbw1, t, a1);
  for (int k = 0; k < 3; ++k) t[k] = G.s * dpv[k] - g[k] * dt * dt / 2;
  mul3v(Rbw1, t, a2);
  for (int k = 0; k < 3; ++k) { err[k] = er[k]; err[3 + k] = a1[k] - dV[k]; err[6 + k] = a2[k] - dP[k]; }
  if (!geom) return;
  for (int k = 0; k < 9; ++k) { geom->Rbw1[k] = Rbw1[k]; geom->eR[k] = eR[k]; }
  for (int k = 0; k < 3; ++k) { geom->dbg[k] = dbg[k]; geom->dv[k] = dv[k]; geom->dpv[k] = dpv[k]; }
}
// e^T Omega e
__device__ __forceinline__ double io_quad(const double* Om, const double* e) {
  double c = 0;
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    double s = 0;
#pragma unroll
    for (int l = 0; l < 9; ++l) s += Om[r * 9 + l] * e[l];
    c += e[r] * s;
  }
  return c;
}
__device__ __forceinline__ double io_huber_rho(double e2) { return e2 <= 1.0 ? e2 : 2.0 * sqrt(e2) - 1.0; }   // RobustKernelHuber, delta 1

// EdgeInertialGS::linearizeOplus, the blocks of the free vertices: J (9 x IO_NC, row-major)
__device__ __forceinline__ void io_link_jacobian(const morb_imu_preintegrated& P, const IoLinkGeom& q, const double* err, const IoGlobal& G,
                                                 bool freeV, bool freeB, bool freeG, bool freeS, double* J) {
#pragma unroll
  for (int k = 0; k < 9 * IO_NC; ++k) J[k] = 0.0;
  const double dt = P.dT, s = G.s;
  if (freeV) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        J[(3 + r) * IO_NC + c] = s * q.Rbw1[r * 3 + c];               // velocity 2
        J[(3 + r) * IO_NC + 3 + c] = -s * q.Rbw1[r * 3 + c];          // velocity 1
        J[(6 + r) * IO_NC + 3 + c] = -s * q.Rbw1[r * 3 + c] * dt;
      }
  }
  if (freeB) {
    double invJr[9], JRg[9], w3[3], rj[9], eRt[9], T[9], T2[9];
    inv_right_jacobian_so3(err, invJr);
    for (int k = 0; k < 9; ++k) JRg[k] = P.JRg[k];
    mul3v(JRg, q.dbg, w3);
    right_jacobian_so3(w3, rj);
    transpose33(q.eR, eRt);
    mul33(invJr, eRt, T); mul33(T, rj, T2); mul33(T2, JRg, T);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        J[r * IO_NC + 6 + c] = -T[r * 3 + c];
        J[(3 + r) * IO_NC + 6 + c] = -(double)P.JVg[r * 3 + c];
        J[(6 + r) * IO_NC + 6 + c] = -(double)P.JPg[r * 3 + c];
        J[(3 + r) * IO_NC + 9 + c] = -(double)P.JVa[r * 3 + c];
        J[(6 + r) * IO_NC + 9 + c] = -(double)P.JPa[r * 3 + c];
      }
  }
  if (freeG) {
    const double G0 = (double)9.81f;
    // dGdTheta = Rwg * [0 -G; G 0; 0 0]: column 0 = G * Rwg[:, 1], column 1 = -G * Rwg[:, 0]
    const double d0[3] = {G.Rwg[1] * G0, G.Rwg[4] * G0, G.Rwg[7] * G0}, d1[3] = {G.Rwg[0] * -G0, G.Rwg[3] * -G0, G.Rwg[6] * -G0};
    double r0[3], r1[3];
    mul3v(q.Rbw1, d0, r0); mul3v(q.Rbw1, d1, r1);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      J[(3 + r) * IO_NC + 12] = -r0[r] * dt; J[(3 + r) * IO_NC + 13] = -r1[r] * dt;
      J[(6 + r) * IO_NC + 12] = -0.5 * r0[r] * dt * dt; J[(6 + r) * IO_NC + 13] = -0.5 * r1[r] * dt * dt;
    }
  }
  if (freeS) {
    double a[3], b[3];
    mul3v(q.Rbw1, q.dv, a); mul3v(q.Rbw1, q.dpv, b);
#pragma unroll
    for (int r = 0; r < 3; ++r) { J[(3 + r) * IO_NC + 14] = a[r]; J[(6 + r) * IO_NC + 14] = b[r]; }
  }
}

// structural non-zeros of J (row l, column c): the rotation rows (0..2) only depend on the gyro bias, velocity 2 only enters the velocity rows
// (3..5).  With constant l and c (unrolled loops) the test folds away and the zero entries cost neither a register nor an operation.
__device__ __forceinline__ constexpr bool io_nz(int l, int c) { return c < 3 ? (l >= 3 && l < 6) : (c >= 6 && c < 9) ? true : l >= 3; }

// entry e of the Schur sum: (i, j <= i) of the corner for e < 45, (i, right-hand side) for 45 <= e < 54
__device__ __forceinline__ void io_entry(int e, int* i, int* j) {
  if (e >= 45) { *i = e - 45; *j = morbarrow::NG; return; }
  int r = 0, t = e;
  while (t > r) { t -= r + 1; ++r; }
  *i = r; *j = t;
}

// GWS: the chain records live in the global workspace (cap > IO_LDS_KF) instead of LDS
template <bool GWS>
__global__ __launch_bounds__(IO_T) void k_inertial_optimization(int cap, const int* __restrict__ kfStart, float* __restrict__ kfState,
                                                                const uint8_t* __restrict__ hasLink,
                                                                const morb_imu_preintegrated* __restrict__ pre, int mode,
                                                                const int* __restrict__ flags, const float* __restrict__ prior2,
                                                                double* __restrict__ global16, uint8_t* __restrict__ reintegrate,
                                                                int* __restrict__ stats4, double* __restrict__ chi2Out,
                                                                double* __restrict__ wsLink, double* __restrict__ wsChain) {
  __shared__ IoShared sh;
  extern __shared__ __align__(16) double sChain[];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int k0 = kfStart[p], n = kfStart[p + 1] - k0;
  double* const chain = GWS ? wsChain + (size_t)p * cap * IO_KS : sChain;
  double* const links = wsLink + (size_t)p * cap * IO_LS;
  float* const st = kfState + (size_t)21 * k0;
  const uint8_t* const hl = hasLink + k0;
  const morb_imu_preintegrated* const P = pre + k0;
  auto linked = [&](int k) { return k >= 1 && k < n && hl[k] != 0; };

  // ---- number of links; a problem without one (or beyond cap) is left alone
  {
    int c = 0;
    if (n >= 2 && n <= cap) for (int k = 1 + tid; k < n; k += IO_T) c += hl[k] != 0 ? 1 : 0;
    c = morbwave::sum_i32(c);
    if (lane == 0) sh.part[wv][0] = (double)c;
    __syncthreads();
    if (tid == 0) sh.nlink = (int)(sh.part[0][0] + sh.part[1][0] + sh.part[2][0] + sh.part[3][0]);
    __syncthreads();
  }
  const int nlink = sh.nlink;
  if (nlink == 0) {
    if (tid == 0) { stats4[4 * p] = 0; stats4[4 * p + 1] = 0; stats4[4 * p + 2] = 0; stats4[4 * p + 3] = 0; }
    return;
  }
  const int fl = flags ? flags[p] : 0;
  const bool lm = mode != 2;
  const bool freeV = mode == 1 || (mode == 0 && !(fl & 2)), freeB = freeV;
  const bool freeG = mode != 1, freeS = mode == 2 || (mode == 0 && (fl & 1));
  const double priorG = lm ? (double)prior2[2 * p] : 0.0, priorA = lm ? (double)prior2[2 * p + 1] : 0.0;

  // ---- set-up: the global unknowns, the velocities, every link's information matrix (EdgeInertialGS's constructor)
  if (tid == 0) {
    const double* g16 = global16 + (size_t)16 * p;
    for (int k = 0; k < 9; ++k) sh.G.Rwg[k] = mode == 1 ? ((k & 3) == 0 ? 1.0 : 0.0) : g16[k];
    sh.G.s = mode == 1 ? 1.0 : g16[9];
    for (int k = 0; k < 3; ++k) { sh.G.bg[k] = g16[10 + k]; sh.G.ba[k] = g16[13 + k]; }
    for (int k = 0; k < 9; ++k) sh.g[k] = 0.0;
  }
  for (int k = tid; k < n; k += IO_T) {
    double* c = chain + (size_t)k * IO_KS;
    for (int r = 0; r < 3; ++r) { c[IO_V + r] = (double)st[21 * k + 12 + r]; c[IO_X + r] = 0.0; }
  }
  // One wave per link: invert_n's Gauss-Jordan inverse with partial pivoting and clamp_eigenvalues' positive-definiteness test
  // (inertial_device.h), element for element the same operations, spread over the lanes on a 9 x 18 LDS tile.  (One thread per link on a global
  // workspace paid ~2 k dependent round trips to memory: half a millisecond at every call.)
  for (int k = 1 + wv; k < n; k += IO_W) {
    if (!linked(k)) continue;   // (wave-uniform)
    double* M = sh.gj[wv];
    double* L = links + (size_t)k * IO_LS;
    double* Info = L + IO_INFO;
    for (int e = lane; e < 162; e += 64) { const int r = e / 18, c = e - r * 18; M[e] = c < 9 ? (double)P[k].C[r * 15 + c] : (c - 9 == r ? 1.0 : 0.0); }
    IO_WAVE_SYNC();
    bool ok = true;
    for (int c = 0; c < 9; ++c) {
      int pv = c;
      for (int r = c + 1; r < 9; ++r) if (fabs(M[r * 18 + c]) > fabs(M[pv * 18 + c])) pv = r;
      const double piv = M[pv * 18 + c];
      if (piv == 0.0) { ok = false; break; }
      IO_WAVE_SYNC();
      if (pv != c && lane < 18) { const double t = M[pv * 18 + lane]; M[pv * 18 + lane] = M[c * 18 + lane]; M[c * 18 + lane] = t; }
      IO_WAVE_SYNC();
      const double inv = 1.0 / piv;
      if (lane < 18) M[c * 18 + lane] *= inv;
      IO_WAVE_SYNC();
      double f[3] = {0, 0, 0}, pr[3] = {0, 0, 0};
#pragma unroll
      for (int q = 0; q < 3; ++q) { const int e = lane + 64 * q; if (e < 162) { const int r = e / 18; f[q] = M[r * 18 + c]; pr[q] = M[c * 18 + (e - r * 18)]; } }
      IO_WAVE_SYNC();
#pragma unroll
      for (int q = 0; q < 3; ++q) { const int e = lane + 64 * q; if (e < 162 && e / 18 != c && f[q] != 0.0) M[e] -= f[q] * pr[q]; }
      IO_WAVE_SYNC();
    }
    if (!ok) { for (int e = lane; e < 81; e += 64) Info[e] = 0.0; continue; }
    double v[2] = {0, 0};
#pragma unroll
    for (int q = 0; q < 2; ++q) {   // Info = (Ainv + Ainv^T) / 2
      const int e = lane + 64 * q;
      if (e < 81) { const int r = e / 9, c = e - r * 9; const double a = M[r * 18 + 9 + c], b = M[c * 18 + 9 + r]; v[q] = r == c ? a : (r < c ? (a + b) / 2 : (b + a) / 2); Info[e] = v[q]; }
    }
    IO_WAVE_SYNC();
#pragma unroll
    for (int q = 0; q < 2; ++q) { const int e = lane + 64 * q; if (e < 81) M[e] = (e % 10 == 0) ? v[q] - 1e-12 : v[q]; }
    IO_WAVE_SYNC();
    bool pd = true;
    for (int j = 0; j < 9; ++j) {   // Info - 1e-12 I positive definite <=> no eigenvalue to clamp
      const double d = M[j * 9 + j];
      if (!(d > 0)) { pd = false; break; }
      double l[2] = {0, 0}, t[2] = {0, 0};
      bool on[2] = {false, false};
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int e = lane + 64 * q, r = e / 9, c = e - r * 9;
        on[q] = e < 81 && c > j && c <= r;
        if (on[q]) { l[q] = M[r * 9 + j] / d; t[q] = M[c * 9 + j]; }
      }
      IO_WAVE_SYNC();
#pragma unroll
      for (int q = 0; q < 2; ++q) if (on[q]) M[lane + 64 * q] -= l[q] * t[q];
      IO_WAVE_SYNC();
    }
    if (!pd && lane == 0) clamp_eigenvalues(Info, 9, 1e-12, L + IO_SCR, L + IO_SCR + 81);   // (rare: the cyclic-Jacobi rebuild, on the link's global scratch)
  }
  __syncthreads();

  // ---- activeRobustChi2 at the current state: per-thread sums over its links, wave sums, the waves in order
  auto chi2_now = [&]() -> double {
    double acc = 0;
    for (int k = 1 + tid; k < n; k += IO_T) {
      if (!linked(k)) continue;
      double e[9];
      io_link_error(P[k], st + 21 * (k - 1), st + 21 * k, chain + (size_t)(k - 1) * IO_KS + IO_V, chain + (size_t)k * IO_KS + IO_V, sh.G, e, nullptr);
      const double c = io_quad(links + (size_t)k * IO_LS + IO_INFO, e);
      acc += lm ? c : io_huber_rho(c);
    }
    acc = morbwave::sum_f64(acc);
    __syncthreads();
    if (lane == 0) sh.red[wv] = acc;
    __syncthreads();
    double tot = sh.red[0] + sh.red[1] + sh.red[2] + sh.red[3];
    if (lm) {   // EdgePriorAcc / EdgePriorGyro: error = 0 - bias, information prior * I
      tot += priorA * (sh.G.ba[0] * sh.G.ba[0] + sh.G.ba[1] * sh.G.ba[1] + sh.G.ba[2] * sh.G.ba[2]);
      tot += priorG * (sh.G.bg[0] * sh.G.bg[0] + sh.G.bg[1] * sh.G.bg[1] + sh.G.bg[2] * sh.G.bg[2]);
    }
    return tot;
  };

  // ---- buildSystem: T, O, F = [B | r] per keyframe, C and rg
  auto build = [&]() {
    for (int c0 = 0; c0 < n; c0 += IO_T) {
      const int k = c0 + tid;
      if (k < n) {
        double* slot = chain + (size_t)k * IO_KS;
        for (int q = 0; q < IO_DINV; ++q) slot[q] = 0.0;
        if (!freeV) slot[IO_T0] = slot[IO_T0 + 4] = slot[IO_T0 + 8] = 1.0;
      }
      if (linked(k)) {
        double* slot = chain + (size_t)k * IO_KS;
        double* L = links + (size_t)k * IO_LS;
        const double* Om = L + IO_INFO;
        double e[9], J[9 * IO_NC], oe[9];
        IoLinkGeom q;
        io_link_error(P[k], st + 21 * (k - 1), st + 21 * k, chain + (size_t)(k - 1) * IO_KS + IO_V, slot + IO_V, sh.G, e, &q);
        io_link_jacobian(P[k], q, e, sh.G, freeV, freeB, freeG, freeS, J);
        double w = 1.0;
        if (!lm) w = huber_w(1.0, io_quad(Om, e));
#pragma unroll
        for (int r = 0; r < 9; ++r) {
          double s = 0;
#pragma unroll
          for (int l = 0; l < 9; ++l) s += Om[r * 9 + l] * e[l];
          oe[r] = w * s;
        }
        int qg = 0;
#pragma unroll
        for (int c = 0; c < IO_NC; ++c) {
          double a[9];
#pragma unroll
          for (int i = 0; i < 9; ++i) {
            double s = 0;
#pragma unroll
            for (int l = 0; l < 9; ++l) if (io_nz(l, c)) s += Om[i * 9 + l] * J[l * IO_NC + c];
            a[i] = w * s;
          }
          double bc = 0;
#pragma unroll
          for (int i = 0; i < 9; ++i) if (io_nz(i, c)) bc += J[i * IO_NC + c] * oe[i];
          bc = -bc;
          if (c < 3) slot[IO_F + c * 10 + 9] = bc;
          else if (c < 6) L[IO_H1 + 36 + (c - 3)] = bc;
          else L[IO_HG + 45 + (c - 6)] = bc;
#pragma unroll
          for (int r = 0; r <= c; ++r) {
            double h = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i) if (io_nz(i, r)) h += J[i * IO_NC + r] * a[i];
            if (c < 3) { slot[IO_T0 + r * 3 + c] = h; slot[IO_T0 + c * 3 + r] = h; }                 // velocity 2 x velocity 2
            else if (c < 6) {
              if (r < 3) slot[IO_O + r * 3 + (c - 3)] = h;                                             // O_k = T(k, k-1): rows velocity 2, columns velocity 1
              else { L[IO_H1 + (r - 3) * 3 + (c - 3)] = h; L[IO_H1 + (c - 3) * 3 + (r - 3)] = h; }   // velocity 1 x velocity 1
            } else {
              if (r < 3) slot[IO_F + r * 10 + (c - 6)] = h;                                            // B_k
              else if (r < 6) L[IO_H1 + 9 + (r - 3) * 9 + (c - 6)] = h;                                // B_{k-1}'s share
              else L[IO_HG + qg++] = h;                                                                // corner, upper triangle by columns
            }
          }
        }
      }
    }
    __syncthreads();
    // the velocity-1 rows of link k + 1 belong to keyframe k (behind the barrier: link k + 1 may be another thread's, or a later pass's)
    if (freeV) for (int k = tid; k < n; k += IO_T) {
      if (!linked(k + 1)) continue;
      double* slot = chain + (size_t)k * IO_KS;
      const double* H1 = links + (size_t)(k + 1) * IO_LS + IO_H1;
      for (int q = 0; q < 9; ++q) slot[IO_T0 + q] += H1[q];
      for (int r = 0; r < 3; ++r) { for (int c = 0; c < 9; ++c) slot[IO_F + r * 10 + c] += H1[9 + r * 9 + c]; slot[IO_F + r * 10 + 9] += H1[36 + r]; }
    }
    __syncthreads();
    // corner and its right-hand side: lane e < 54 of wave w sums entry e over the w-th quarter of the links, in link order
    {
      const int per = (n + IO_W - 1) / IO_W, ka = wv * per, kb = min(n, ka + per);
      double s = 0;
      if (lane < 54) for (int k = max(ka, 1); k < kb; ++k) if (linked(k)) s += links[(size_t)k * IO_LS + IO_HG + lane];
      if (lane < 54) sh.part[wv][lane] = s;
      __syncthreads();
      if (tid < 54) {
        const double tot = sh.part[0][tid] + sh.part[1][tid] + sh.part[2][tid] + sh.part[3][tid];
        if (tid < 45) {   // upper triangle by columns: entry q = c (c + 1) / 2 + r of (r <= c)
          int c = 0, r = tid;
          while (r > c) { r -= c + 1; ++c; }
          sh.C[r * 9 + c] = tot; sh.C[c * 9 + r] = tot;
        } else sh.rg[tid - 45] = tot;
      }
      __syncthreads();
      if (tid == 0) {
        if (lm) for (int r = 0; r < 3; ++r) {
          if (freeB) { sh.C[r * 10] += priorG; sh.C[(3 + r) * 10] += priorA; sh.rg[r] -= priorG * sh.G.bg[r]; sh.rg[3 + r] -= priorA * sh.G.ba[r]; }
        }
        for (int r = 0; r < 9; ++r) {
          const bool fr = r < 6 ? freeB : (r < 8 ? freeG : freeS);
          if (!fr) { for (int c = 0; c < 9; ++c) { sh.C[r * 9 + c] = 0.0; sh.C[c * 9 + r] = 0.0; } sh.C[r * 10] = 1.0; sh.rg[r] = 0.0; }
        }
      }
      __syncthreads();
    }
  };

  // ---- solve with lambda on every diagonal; sh.flag = the factorisation succeeded; x per keyframe, sh.g
  auto solve = [&](double lambda) {
    if (tid == 0) sh.flag = 1;
    __syncthreads();
    if (freeV) {
      if (wv == 0) {
        bool ok = true;
        double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, DinvPrev[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, col[3] = {0, 0, 0};
        for (int k = 0; k < n; ++k) {
          double* slot = chain + (size_t)k * IO_KS;
          const bool first = k == 0;
          double Tk[9], Ok[9], Dinv[9];
#pragma unroll
          for (int q = 0; q < 9; ++q) { Tk[q] = slot[IO_T0 + q]; Ok[q] = slot[IO_O + q]; }
          if (!first) morbarrow::chain_multiplier(Ok, DinvPrev, M);
          if (!morbarrow::chain_pivot(Tk, lambda, first, M, Ok, Dinv)) { ok = false; break; }   // (uniform: every lane computes the same block)
          if (lane < morbarrow::NF) {
            const double f[3] = {slot[IO_F + lane], slot[IO_F + 10 + lane], slot[IO_F + 20 + lane]};
            morbarrow::chain_forward_column(f, first, M, col);
            slot[IO_FP + lane] = col[0]; slot[IO_FP + 10 + lane] = col[1]; slot[IO_FP + 20 + lane] = col[2];
          }
          if (lane == 0) for (int q = 0; q < 9; ++q) slot[IO_DINV + q] = Dinv[q];
#pragma unroll
          for (int q = 0; q < 9; ++q) DinvPrev[q] = Dinv[q];
        }
        if (!ok && lane == 0) sh.flag = 0;
      }
      __syncthreads();
    }
    if (sh.flag) {
      // Schur complement: lane e < 54 of wave w sums entry e over the w-th quarter of the keyframes, in order
      const int per = (n + IO_W - 1) / IO_W, ka = wv * per, kb = min(n, ka + per);
      int ei = 0, ej = 0;
      io_entry(lane < 54 ? lane : 0, &ei, &ej);
      double s = 0;
      if (freeV && lane < 54) for (int k = ka; k < kb; ++k) s += morbarrow::schur_term(chain + (size_t)k * IO_KS + IO_FP, chain + (size_t)k * IO_KS + IO_DINV, ei, ej);
      if (lane < 54) sh.part[wv][lane] = s;
      __syncthreads();
      if (tid < 54) {
        const double tot = sh.part[0][tid] + sh.part[1][tid] + sh.part[2][tid] + sh.part[3][tid];
        if (tid < 45) sh.S[ei * 9 + ej] = sh.C[ei * 9 + ej] + (ei == ej ? lambda : 0.0) - tot;
        else sh.rhs[ei] = sh.rg[ei] - tot;
      }
      __syncthreads();
      if (tid == 0 && !morbarrow::corner_solve(sh.S, sh.rhs, sh.g)) sh.flag = 0;
      __syncthreads();
    }
    if (sh.flag && freeV) {
      for (int k = tid; k < n; k += IO_T) morbarrow::back_rhs(chain + (size_t)k * IO_KS + IO_FP, sh.g, chain + (size_t)k * IO_KS + IO_X);
      __syncthreads();
      if (tid == 0) {
        double xn[3] = {0, 0, 0};
        for (int k = n - 1; k >= 0; --k) {
          double* slot = chain + (size_t)k * IO_KS;
          const bool last = k == n - 1;
          const double y[3] = {slot[IO_X], slot[IO_X + 1], slot[IO_X + 2]};
          double x[3];
          morbarrow::chain_back(slot + IO_DINV, y, last, last ? slot : slot + IO_KS + IO_O, xn, x);
          for (int r = 0; r < 3; ++r) { slot[IO_X + r] = x[r]; xn[r] = x[r]; }
        }
      }
    }
    __syncthreads();
    if (!sh.flag) {   // a failed factorisation: a zero step, which the caller rejects (LM) or stops at (Gauss-Newton)
      for (int k = tid; k < n; k += IO_T) for (int r = 0; r < 3; ++r) chain[(size_t)k * IO_KS + IO_X + r] = 0.0;
      if (tid < 9) sh.g[tid] = 0.0;
      __syncthreads();
    }
  };

  // ---- push, oplus, pop
  auto apply = [&]() {
    if (freeV) for (int k = tid; k < n; k += IO_T) {
      double* slot = chain + (size_t)k * IO_KS;
      for (int r = 0; r < 3; ++r) { slot[IO_VBK + r] = slot[IO_V + r]; slot[IO_V + r] += slot[IO_X + r]; }
    }
    if (tid == 0) {
      sh.Gbk = sh.G;
      for (int r = 0; r < 3; ++r) { sh.G.bg[r] += sh.g[r]; sh.G.ba[r] += sh.g[3 + r]; }
      const double u[3] = {sh.g[6], sh.g[7], 0.0};
      double dR[9], R[9];
      exp_so3(u, dR);
      for (int q = 0; q < 9; ++q) R[q] = sh.G.Rwg[q];
      mul33(R, dR, R);
      for (int q = 0; q < 9; ++q) sh.G.Rwg[q] = R[q];
      const double us = sh.g[8];
      sh.G.s = sh.G.s * (fabs(us) < 512.0 ? morbm64::exp_glibc(us) : exp(us));
    }
    __syncthreads();
  };
  auto restore = [&]() {
    if (freeV) for (int k = tid; k < n; k += IO_T) {
      double* slot = chain + (size_t)k * IO_KS;
      for (int r = 0; r < 3; ++r) slot[IO_V + r] = slot[IO_VBK + r];
    }
    if (tid == 0) sh.G = sh.Gbk;
    __syncthreads();
  };
  // computeScale: sum x (lambda x + b)
  auto gain = [&](double lambda) -> double {
    double acc = 0;
    if (freeV) for (int k = tid; k < n; k += IO_T) {
      const double* slot = chain + (size_t)k * IO_KS;
      for (int r = 0; r < 3; ++r) acc += slot[IO_X + r] * (lambda * slot[IO_X + r] + slot[IO_F + r * 10 + 9]);
    }
    acc = morbwave::sum_f64(acc);
    __syncthreads();
    if (lane == 0) sh.red[wv] = acc;
    __syncthreads();
    double tot = sh.red[0] + sh.red[1] + sh.red[2] + sh.red[3];
    for (int r = 0; r < 9; ++r) tot += sh.g[r] * (lambda * sh.g[r] + sh.rg[r]);
    return tot;
  };

  int its = 0, trials = 0, okFlag = 1;
  const double chiBefore = chi2_now();
  double chiAfter = chiBefore;
  if (lm) {
    LmControl c;
    const double userLambda = (mode == 1 || priorG != 0.0) ? 1e3 : 0.0;
    for (int iter = 0; iter < 200; ++iter) {
      ++its;
      lm_iteration(c, iter == 0 ? chiBefore : chi2_now());
      build();
      if (iter == 0) {
        double m = 0;
        if (freeV) for (int k = tid; k < n; k += IO_T) for (int r = 0; r < 3; ++r) m = fmax(m, fabs(chain[(size_t)k * IO_KS + IO_T0 + r * 4]));
        for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
        __syncthreads();
        if (lane == 0) sh.red[wv] = m;
        __syncthreads();
        m = fmax(fmax(sh.red[0], sh.red[1]), fmax(sh.red[2], sh.red[3]));
        for (int r = 0; r < 9; ++r) { const bool fr = r < 6 ? freeB : (r < 8 ? freeG : freeS); if (fr) m = fmax(m, fabs(sh.C[r * 10])); }
        lm_begin(c, userLambda, m);
      }
      bool again = true;
      while (again) {   // at most ten trials: lm_trial counts them
        solve(c.lambda);
        const bool ok2 = sh.flag != 0;
        apply();
        const double tempChi = chi2_now();
        const double gn = gain(c.lambda);
        const bool keep = lm_trial(c, tempChi, ok2, gn, &again);
        if (!keep) restore();
        ++trials;
      }
      if (lm_iteration_done(c)) break;
    }
    chiAfter = c.currentChi;
  } else {
    for (int iter = 0; iter < 10; ++iter) {
      ++its;
      build();
      solve(0.0);
      const bool ok2 = sh.flag != 0;
      apply();
      if (!ok2) { okFlag = 0; break; }
    }
    chiAfter = chi2_now();
  }
  __syncthreads();

  // ---- write-back
  if (lm) {
    const float bgf[3] = {(float)sh.G.bg[0], (float)sh.G.bg[1], (float)sh.G.bg[2]}, baf[3] = {(float)sh.G.ba[0], (float)sh.G.ba[1], (float)sh.G.ba[2]};
    for (int k = tid; k < n; k += IO_T) {
      float* s0 = st + 21 * k;
      const float d0 = s0[15] - bgf[0], d1 = s0[16] - bgf[1], d2 = s0[17] - bgf[2];
      const float nrm = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
      reintegrate[k0 + k] = ((double)nrm > 0.01 && linked(k)) ? 1 : 0;
      for (int r = 0; r < 3; ++r) { s0[12 + r] = (float)chain[(size_t)k * IO_KS + IO_V + r]; s0[15 + r] = bgf[r]; s0[18 + r] = baf[r]; }
    }
  }
  if (tid == 0) {
    double* g16 = global16 + (size_t)16 * p;
    if (mode != 1) { for (int k = 0; k < 9; ++k) g16[k] = sh.G.Rwg[k]; g16[9] = sh.G.s; }
    if (mode != 2) for (int k = 0; k < 3; ++k) { g16[10 + k] = sh.G.bg[k]; g16[13 + k] = sh.G.ba[k]; }
    stats4[4 * p] = its; stats4[4 * p + 1] = trials; stats4[4 * p + 2] = okFlag; stats4[4 * p + 3] = nlink;
    chi2Out[2 * p] = chiBefore; chi2Out[2 * p + 1] = chiAfter;
  }
}

}  // namespace

extern "C" int morb_inertial_optimization_batch(morb_optimizer* o, int nprob, int cap, const int* d_kfStart, float* d_kfState21,
                                                const uint8_t* d_hasLink, const morb_imu_preintegrated* d_pre, int mode, const int* d_flags,
                                                const float* d_prior2, double* d_global16, uint8_t* d_reintegrate, int* d_stats4,
                                                double* d_chi2, void* stream) {
  MORB_REQUIRE(o && d_kfStart && d_kfState21 && d_hasLink && d_pre && d_global16 && d_stats4 && d_chi2, MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(mode >= 0 && mode <= 2, MORB_ERR_INVALID, "mode must be 0, 1 or 2");
  MORB_REQUIRE(mode == 2 || (d_prior2 && d_reintegrate), MORB_ERR_INVALID, "modes 0 and 1 need d_prior2 and d_reintegrate");
  MORB_REQUIRE(mode != 0 || d_flags, MORB_ERR_INVALID, "mode 0 needs d_flags");
  MORB_REQUIRE(nprob > 0 && cap > 0, MORB_ERR_INVALID, "bad sizes");
  MORB_REQUIRE(cap <= IO_MAX_KF, MORB_ERR_CAPACITY, "more than 4096 keyframes in one problem");
  MORB_ENTER(st, o, stream);
  const bool gws = cap > IO_LDS_KF;
  const size_t nLink = (size_t)nprob * cap * IO_LS, nChain = gws ? (size_t)nprob * cap * IO_KS : 0;
  double* ws = nullptr;
  { const int rc = grow(o->inertialOpt, nLink + nChain, &ws); if (rc != MORB_OK) return rc; }
  if (gws) {
    hipLaunchKernelGGL(k_inertial_optimization<true>, dim3(nprob), dim3(IO_T), 0, st, cap, d_kfStart, d_kfState21, d_hasLink, d_pre, mode, d_flags,
                       d_prior2, d_global16, d_reintegrate, d_stats4, d_chi2, ws, ws + nLink);
  } else {
    const size_t lds = (size_t)cap * IO_KS * sizeof(double);
    MORB_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_inertial_optimization<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_inertial_optimization<false>, dim3(nprob), dim3(IO_T), lds, st, cap, d_kfStart, d_kfState21, d_hasLink, d_pre, mode, d_flags,
                       d_prior2, d_global16, d_reintegrate, d_stats4, d_chi2, ws, (double*)nullptr);
  }
  MORB_HIP_CHECK(hipGetLastError());
  return MORB_OK;
}
