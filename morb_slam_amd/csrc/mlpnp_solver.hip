// MLPnPsolver (reference src/MLPnPsolver.cpp) for MI355X (gfx950), batched: one 256-thread workgroup per problem (a frame and the map
// points one relocalisation candidate matched to it).  Each call restates
//   * the constructor (:55-97): the kept matches compacted in feature order (ransac_block.h), bearing vectors unproject(kp.pt) / z
//     in float (unproject of morb/camera_math.h: Pinhole, or KannalaBrandt8's Newton unprojection), world points, sigma2;
//   * SetRansacParameters (:225-260) from the device-side N (include/morb/mlpnp_solver_math.h, ransac_math.h);
//   * iterate (:100-223) from state.iterations on: DUtils::Random::RandomInt + swap-with-back sampling on the caller's rand() values
//     (minSet per iteration, indexed by the global iteration number), computePose (:356-658) in FP64, CheckInliers (:262-293) in
//     float, the running best, Refine() on the BEST mask after every iteration that reaches minInliers, the post-loop best branch.
// Mapping: the correspondences (10 words each) live in LDS up to MP_LDS_N, in the handle's mlpnpCorr workspace beyond.  Hypotheses
// are built MP_G at a time, speculatively (sampling depends only on the rand() stream and N): a row of 16 lanes per hypothesis,
// its 12 x 12 normal matrix and eigenvector matrix resident in LDS, lane k owning row / column k of a Jacobi rotation (row_jacobi.h); the six
// residual rows of the Gauss-Newton are one lane each.  Their inliers are counted one wave per hypothesis (ballots), then the
// reference's rule is applied in iteration order, so nothing after the first success is reported.  Refine() runs the same
// 16-lane routine over the best inliers, 16 correspondences at a time.  The numerical choices Eigen made for the reference
// (Jacobi, rank, null-space basis, sum orders, the hand-derived Jacobian) are DESIGN.md section 6, "MLPnPsolver".
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "handles.h"
#include "morb/camera_math.h"
#include "libm_f32.h"
#include "morb_hip.h"
#include "morb/mlpnp_solver_math.h"
#include "morb/ransac_math.h"
#include "ransac_block.h"
#include "row_jacobi.h"

#ifndef MORB_MLPNP_THREADS
#define MORB_MLPNP_THREADS 256
#endif

namespace {

constexpr int MP_NT = MORB_MLPNP_THREADS;
constexpr int MP_NW = MP_NT / 64;
constexpr int MP_GL = morbrow::ROW_LANES;   // lanes per hypothesis
constexpr int MP_G = MP_NT / MP_GL;    // hypotheses built per batch
constexpr int MP_LDS_N = 384;          // correspondences held in LDS; beyond, the global workspace
constexpr int MP_W = 10;               // words per correspondence
constexpr int MP_MAXSET = 16;          // largest minSet
constexpr double MP_EPS = 2.220446049250313e-16;
static_assert(MP_NT % 64 == 0 && MP_NT >= 64, "whole waves");

using morbcam::Camera;
using namespace morbransac;
using morbrow::g_jacobi;

struct Corr {   // structure of arrays, `stride` entries each
  float *X, *uv, *err, *br;
  int *id, *list;
  int stride;
};
__device__ inline Corr mp_carve(float* base, int stride) {
  Corr c;
  c.X = base; c.uv = base + 3 * stride; c.err = base + 5 * stride; c.br = base + 6 * stride;
  c.id = (int*)(base + 8 * stride); c.list = (int*)(base + 9 * stride);
  c.stride = stride;
  return c;
}

struct Grp {   // the LDS of one 16-lane row
  double W[288];           // A = W (m x m, row-major), V = W + 144; the Gauss-Newton's residual rows afterwards
  double x[12];            // the null vector
  double Er[9];            // eigenRot
  double R[9], t[3];       // the pose this row computed
  double red[MP_GL];
  int idx[MP_MAXSET], pos[MP_MAXSET], val[MP_MAXSET];
};

struct MpShared {
  float corr[MP_LDS_N * MP_W];
  Grp grp[MP_G];
  int cnt[MP_G];
  int wcount[MP_NW];
  int N, nc, iters, bestInliers, improved, done, refFail, nList, nRef;
  float bestTcw[12];
};

__device__ __forceinline__ void load_point(const Corr& C, int i, double* X, double* f) {
  const int S = C.stride;
  X[0] = (double)C.X[i]; X[1] = (double)C.X[S + i]; X[2] = (double)C.X[2 * S + i];
  f[0] = (double)C.br[i]; f[1] = (double)C.br[S + i]; f[2] = 1.0;
}

// orthonormal basis (r, s) of the complement of f: Nb[a * 2 + c]
__device__ __forceinline__ void null_basis(const double* f, double* Nb) {
  const double n = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
  const double ux = f[0] / n, uy = f[1] / n, uz = f[2] / n;
  const double a = 1.0 / (1.0 + uz), b = -ux * uy * a;
  Nb[0] = 1.0 - ux * ux * a; Nb[2] = b; Nb[4] = -ux;
  Nb[1] = b; Nb[3] = 1.0 - uy * uy * a; Nb[5] = -uy;
}

__device__ __forceinline__ double det3(const double* M) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

__device__ __forceinline__ void rodrigues2rot(const double* w, double* R) {
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  if (th > MP_EPS) {
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    const double a = sin(th) / th, b = (1 - cos(th)) / (th * th);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double k2 = K[i * 3] * K[j] + K[i * 3 + 1] * K[3 + j] + K[i * 3 + 2] * K[6 + j];
        R[i * 3 + j] = R[i * 3 + j] + a * K[i * 3 + j] + b * k2;
      }
  }
}

__device__ __forceinline__ void rot2rodrigues(const double* R, double* w) {
  w[0] = 0.0; w[1] = 0.0; w[2] = 0.0;
  const double trace = R[0] + R[4] + R[8] - 1.0;
  const double wnorm = acos(trace / 2.0);
  if (wnorm > MP_EPS) {
    const double sc = wnorm / (2.0 * sin(wnorm));
    w[0] = (R[7] - R[5]) * sc;
    w[1] = (R[2] - R[6]) * sc;
    w[2] = (R[3] - R[1]) * sc;
  }
}

// r = N^T normalize(R(w) X + T) and J = dr / d(w, T) (J[c * 6 + a]), the Jacobian derived by hand:
// dy/dp = (I - y y^T) / |p|, dp/dT = I, dp/dw = -R [X]x (w w^T + (R^T - I) [w]x) / |w|^2, and -[X]x for |w| <= 1e-8
__device__ __forceinline__ void residual_jac(const double* x, const double* R, const double* X, const double* Nb, double* r, double* J) {
  double p[3], y[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = R[i * 3] * X[0] + R[i * 3 + 1] * X[1] + R[i * 3 + 2] * X[2] + x[3 + i];
  const double n = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = p[i] / n;
#pragma unroll
  for (int c = 0; c < 2; ++c) r[c] = Nb[c] * y[0] + Nb[2 + c] * y[1] + Nb[4 + c] * y[2];
  double G[9];
  const double th2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
  const double Xx[9] = {0.0, -X[2], X[1], X[2], 0.0, -X[0], -X[1], X[0], 0.0};
  if (sqrt(th2) <= 1e-8) {
#pragma unroll
    for (int i = 0; i < 9; ++i) G[i] = -Xx[i];
  } else {
    const double Wx[9] = {0.0, -x[2], x[1], x[2], 0.0, -x[0], -x[1], x[0], 0.0};
    double Q[9], RX[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) s += (R[k * 3 + i] - (k == i ? 1.0 : 0.0)) * Wx[k * 3 + j];
        Q[i * 3 + j] = (x[i] * x[j] + s) / th2;
        RX[i * 3 + j] = R[i * 3] * Xx[j] + R[i * 3 + 1] * Xx[3 + j] + R[i * 3 + 2] * Xx[6 + j];
      }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) G[i * 3 + j] = -(RX[i * 3] * Q[j] + RX[i * 3 + 1] * Q[3 + j] + RX[i * 3 + 2] * Q[6 + j]);
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    double d[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) d[j] = (Nb[j * 2 + c] - r[c] * y[j]) / n;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      J[c * 6 + j] = d[0] * G[j] + d[1] * G[3 + j] + d[2] * G[6 + j];
      J[c * 6 + 3 + j] = d[j];
    }
  }
}

// 6 x 6 LDL^T without pivoting, A row-major; false when a value of the solution is not finite
__device__ __forceinline__ bool ldlt6_solve(const double* A, const double* g, double* x) {
  double L[36], D[6], z[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[j * 6 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j * 6 + k] * L[j * 6 + k] * D[k];
    D[j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i * 6 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i * 6 + k] * L[j * 6 + k] * D[k];
      L[i * 6 + j] = s / d;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i * 6 + k] * z[k];
    z[i] = s;
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = z[i] / D[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= L[k * 6 + i] * x[k];
    x[i] = s;
  }
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 6; ++i) ok = ok && (fabs(x[i]) <= 1.79769313486231570815e308);
  return ok;
}

// U V^T of the SVD of M = M (M^T M)^-1/2, negated when its determinant is negative; every lane of the row returns it
__device__ __forceinline__ void g_nearest_rotation(Grp& g, const double* M, int l, double* R) {
  if (l < 9) {
    const int i = l / 3, j = l % 3;
    g.W[l] = M[i] * M[j] + M[3 + i] * M[3 + j] + M[6 + i] * M[6 + j];
  }
  MORB_ROW_SYNC();
  g_jacobi(g.W, g.W + 144, g.red, 3, l);
  const double* V = g.W + 144;
  const double w[3] = {1.0 / sqrt(g.W[0]), 1.0 / sqrt(g.W[4]), 1.0 / sqrt(g.W[8])};
  double S[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) S[i * 3 + j] = V[i * 3] * w[0] * V[j * 3] + V[i * 3 + 1] * w[1] * V[j * 3 + 1] + V[i * 3 + 2] * w[2] * V[j * 3 + 2];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = M[i * 3] * S[j] + M[i * 3 + 1] * S[3 + j] + M[i * 3 + 2] * S[6 + j];
  if (det3(R) < 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = -R[i];
  }
  MORB_ROW_SYNC();
}

// sum over the first six correspondences of 1 - normalize(R X + t) . f (the un-normalised bearing vector)
__device__ __forceinline__ double repro6(const Corr& C, const int* list, const double* R, const double* t) {
  double s = 0;
  for (int p = 0; p < 6; ++p) {
    double X[3], f[3], v[3];
    load_point(C, list[p], X, f);
#pragma unroll
    for (int r = 0; r < 3; ++r) v[r] = R[r * 3] * X[0] + R[r * 3 + 1] * X[1] + R[r * 3 + 2] * X[2] + t[r];
    const double nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    s += 1.0 - (v[0] / nv * f[0] + v[1] / nv * f[1] + v[2] / nv * f[2]);
  }
  return s;
}

// MLPnPsolver::computePose (:356-658) over the n correspondences list[0 .. n), by the 16 lanes of one row; the pose goes to g.R / g.t
__device__ __forceinline__ void g_compute_pose(Grp& g, const Corr& C, const int* list, int n, int l) {
  // ---- planar test: rank of P P^T ----
  if (l < 9) {
    const int i = l / 3, j = l % 3, S = C.stride;
    double s = 0;
    for (int k = 0; k < n; ++k) {
      const int c = list[k];
      s += (double)C.X[i * S + c] * (double)C.X[j * S + c];
    }
    g.W[l] = s;
  }
  MORB_ROW_SYNC();
  g_jacobi(g.W, g.W + 144, g.red, 3, l);
  bool planar;
  {
    const double e0 = g.W[0], e1 = g.W[4], e2 = g.W[8];
    double big = 0;
    big = fabs(e0) > big ? fabs(e0) : big;
    big = fabs(e1) > big ? fabs(e1) : big;
    big = fabs(e2) > big ? fabs(e2) : big;
    const double thr = big * MP_EPS * 3.0;
    const int rank = (fabs(e0) > thr) + (fabs(e1) > thr) + (fabs(e2) > thr);
    planar = rank == 2;
    if (planar) {   // eigenvectors by increasing eigenvalue (a stable sort of three)
      int o0 = 0, o1 = 1, o2 = 2;
      double v0 = e0, v1 = e1, v2 = e2;
      if (v1 < v0) { const int ti = o0; o0 = o1; o1 = ti; const double tv = v0; v0 = v1; v1 = tv; }
      if (v2 < v1) { const int ti = o1; o1 = o2; o2 = ti; const double tv = v1; v1 = v2; v2 = tv; }
      if (v1 < v0) { const int ti = o0; o0 = o1; o1 = ti; const double tv = v0; v0 = v1; v1 = tv; }
      if (l < 9) {
        const int r = l / 3, c = l % 3;
        const int o = r == 0 ? o0 : (r == 1 ? o1 : o2);
        g.Er[l] = g.W[144 + c * 3 + o];
      }
    }
  }
  MORB_ROW_SYNC();
  const int m = planar ? 9 : 12;
  // ---- A^T A: lane j sums column j over the correspondences in list order, row r then row s of each ----
  {
    double acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.0;
    double Er[9];
    if (planar) {
#pragma unroll
      for (int i = 0; i < 9; ++i) Er[i] = g.Er[i];
    }
    for (int k = 0; k < n; ++k) {
      double X[3], f[3], Nb[6], Y[3];
      load_point(C, list[k], X, f);
      null_basis(f, Nb);
      if (planar) {
#pragma unroll
        for (int r = 0; r < 3; ++r) Y[r] = Er[r * 3] * X[0] + Er[r * 3 + 1] * X[1] + Er[r * 3 + 2] * X[2];
      } else {
        Y[0] = X[0]; Y[1] = X[1]; Y[2] = X[2];
      }
#pragma unroll
      for (int row = 0; row < 2; ++row) {
        double e[12];
        if (planar) {
#pragma unroll
          for (int c = 0; c < 6; ++c) e[c] = Nb[(c / 2) * 2 + row] * Y[1 + c % 2];
#pragma unroll
          for (int c = 6; c < 9; ++c) e[c] = Nb[(c - 6) * 2 + row];
          e[9] = 0.0; e[10] = 0.0; e[11] = 0.0;
        } else {
#pragma unroll
          for (int c = 0; c < 9; ++c) e[c] = Nb[(c / 3) * 2 + row] * Y[c % 3];
#pragma unroll
          for (int c = 9; c < 12; ++c) e[c] = Nb[(c - 9) * 2 + row];
        }
        double ej = 0.0;
#pragma unroll
        for (int c = 0; c < 12; ++c) ej = (c == l) ? e[c] : ej;
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] += e[i] * ej;
      }
    }
    if (l < m) {
#pragma unroll
      for (int i = 0; i < 12; ++i)
        if (i < m) g.W[i * m + l] = acc[i];
    }
  }
  MORB_ROW_SYNC();
  g_jacobi(g.W, g.W + 144, g.red, m, l);
  {
    int kmin = 0;
    double best = fabs(g.W[0]);
    for (int k = 1; k < m; ++k) {
      const double v = fabs(g.W[k * m + k]);
      if (v < best) { best = v; kmin = k; }
    }
    if (l < m) g.x[l] = g.W[144 + l * m + kmin];
  }
  MORB_ROW_SYNC();
  double x[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) x[k] = g.x[k];
  double Rout[9], tout[3];
  if (planar) {
    const double c1[3] = {x[0], x[2], x[4]}, c2[3] = {x[1], x[3], x[5]};
    double T[9];   // rows: c1 x c2, c1, c2
    T[0] = c1[1] * c2[2] - c1[2] * c2[1];
    T[1] = c1[2] * c2[0] - c1[0] * c2[2];
    T[2] = c1[0] * c2[1] - c1[1] * c2[0];
#pragma unroll
    for (int a = 0; a < 3; ++a) { T[3 + a] = c1[a]; T[6 + a] = c2[a]; }
    const double n1 = sqrt(T[1] * T[1] + T[4] * T[4] + T[7] * T[7]);
    const double n2 = sqrt(T[2] * T[2] + T[5] * T[5] + T[8] * T[8]);
    const double scale = 1.0 / sqrt(fabs(n1 * n2));
    double Rn[9], R1[9], R2[9], Er[9];
    g_nearest_rotation(g, T, l, Rn);
#pragma unroll
    for (int i = 0; i < 9; ++i) Er[i] = g.Er[i];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R1[i * 3 + j] = -(Er[j] * Rn[i] + Er[3 + j] * Rn[3 + i] + Er[6 + j] * Rn[6 + i]);
    if (det3(R1) < 0) { R1[2] = -R1[2]; R1[5] = -R1[5]; R1[8] = -R1[8]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) { R2[i * 3] = -R1[i * 3]; R2[i * 3 + 1] = -R1[i * 3 + 1]; R2[i * 3 + 2] = R1[i * 3 + 2]; }
    const double t[3] = {scale * x[6], scale * x[7], scale * x[8]}, tn[3] = {-t[0], -t[1], -t[2]};
    const double nv0 = repro6(C, list, R1, t), nv1 = repro6(C, list, R1, tn), nv2 = repro6(C, list, R2, t), nv3 = repro6(C, list, R2, tn);
    int best = 0;
    double bv = nv0;
    if (nv1 < bv) { bv = nv1; best = 1; }
    if (nv2 < bv) { bv = nv2; best = 2; }
    if (nv3 < bv) { bv = nv3; best = 3; }
#pragma unroll
    for (int i = 0; i < 9; ++i) Rout[i] = best < 2 ? R1[i] : R2[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tout[i] = (best & 1) ? tn[i] : t[i];
  } else {
    double Mt[9], Rn[9];   // the transpose of the row-major 3 x 3 of x
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Mt[i * 3 + j] = x[3 * j + i];
    double cn[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) cn[j] = sqrt(Mt[j] * Mt[j] + Mt[3 + j] * Mt[3 + j] + Mt[6 + j] * Mt[6 + j]);
    const double scale = 1.0 / cbrt(fabs(cn[0] * cn[1] * cn[2]));
    g_nearest_rotation(g, Mt, l, Rn);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Rout[i * 3 + j] = Rn[j * 3 + i];
    const double tp[3] = {scale * x[9], scale * x[10], scale * x[11]}, tm[3] = {-tp[0], -tp[1], -tp[2]};
    const double e0 = repro6(C, list, Rout, tm), e1 = repro6(C, list, Rout, tp);
#pragma unroll
    for (int i = 0; i < 3; ++i) tout[i] = e0 < e1 ? tm[i] : tp[i];
  }
  // ---- Gauss-Newton (:694-758): lane k computes the residual rows of correspondence base + k, lane e sums entries e, e + 16, e + 32
  // of (J^T J | J^T r) over the correspondences in list order ----
  double xs[6];
  rot2rodrigues(Rout, xs);
  xs[3] = tout[0]; xs[4] = tout[1]; xs[5] = tout[2];
  for (int it = 0; it < 5; ++it) {
    double R[9];
    rodrigues2rot(xs, R);
    double acc[3] = {0.0, 0.0, 0.0};
    int ia[3], ib[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int e = l + 16 * u;   // e < 36: J^T J (e / 6, e % 6); 36 .. 41: J^T r (e - 36); beyond: unused
      ia[u] = e < 36 ? e / 6 : (e < 42 ? e - 36 : 0);
      ib[u] = e < 36 ? e % 6 : (e < 42 ? 12 : 0);
    }
    for (int base = 0; base < n; base += MP_GL) {
      const int k = base + l;
      if (k < n) {
        double X[3], f[3], Nb[6], r[2], J[12];
        load_point(C, list[k], X, f);
        null_basis(f, Nb);
        residual_jac(xs, R, X, Nb, r, J);
        double* w = g.W + l * 14;
#pragma unroll
        for (int a = 0; a < 12; ++a) w[a] = J[a];
        w[12] = r[0]; w[13] = r[1];
      }
      MORB_ROW_SYNC();
      const int cnt = min(MP_GL, n - base);
      for (int kk = 0; kk < cnt; ++kk) {
        const double* w = g.W + kk * 14;
#pragma unroll
        for (int row = 0; row < 2; ++row)
#pragma unroll
          for (int u = 0; u < 3; ++u) {
            const double b = ib[u] == 12 ? w[12 + row] : w[row * 6 + ib[u]];
            acc[u] += w[row * 6 + ia[u]] * b;
          }
      }
      MORB_ROW_SYNC();
    }
#pragma unroll
    for (int u = 0; u < 3; ++u)
      if (l + 16 * u < 42) g.W[l + 16 * u] = acc[u];
    MORB_ROW_SYNC();
    double A[36], gv[6], dx[6];
#pragma unroll
    for (int e = 0; e < 36; ++e) A[e] = g.W[e];
#pragma unroll
    for (int e = 0; e < 6; ++e) gv[e] = g.W[36 + e];
    MORB_ROW_SYNC();
    if (!ldlt6_solve(A, gv, dx)) break;
    double mx = 0, mn = 1e300;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double v = fabs(dx[a]);
      mx = mx < v ? v : mx;
      mn = v < mn ? v : mn;
    }
    if (mx > 5.0 || mn > 1.0) break;
    double dl = 0;
    for (int base = 0; base < n; base += MP_GL) {
      const int k = base + l;
      if (k < n) {
        double X[3], f[3], Nb[6], r[2], J[12];
        load_point(C, list[k], X, f);
        null_basis(f, Nb);
        residual_jac(xs, R, X, Nb, r, J);
#pragma unroll
        for (int row = 0; row < 2; ++row) {
          double s = 0;
#pragma unroll
          for (int a = 0; a < 6; ++a) s += J[row * 6 + a] * dx[a];
          const double v = fabs(s);
          dl = dl < v ? v : dl;
        }
      }
    }
    g.red[l] = dl;
    MORB_ROW_SYNC();
    dl = 0;
    for (int j = 0; j < MP_GL; ++j) dl = dl < g.red[j] ? g.red[j] : dl;
    MORB_ROW_SYNC();
#pragma unroll
    for (int a = 0; a < 6; ++a) xs[a] -= dx[a];
    if (dl < 1e-5) break;
  }
  double R[9];
  rodrigues2rot(xs, R);
  if (l < 9) g.R[l] = R[l];
  if (l < 3) g.t[l] = xs[3 + l];
  MORB_ROW_SYNC();
}

struct Pose { double R[9], t[3]; };

// CheckInliers' test of correspondence i (:265-292): R X + t in double, rounded to float, projected in float
__device__ __forceinline__ bool is_inlier(const Corr& C, int i, const Pose& P, const Camera& cam) {
  const int S = C.stride;
  const double x = (double)C.X[i], y = (double)C.X[S + i], z = (double)C.X[2 * S + i];
  float Pc[3], uv[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) Pc[r] = (float)(P.R[r * 3] * x + P.R[r * 3 + 1] * y + P.R[r * 3 + 2] * z + P.t[r]);
  morbcam::project(cam, Pc, uv[0], uv[1]);
  const float dx = C.uv[i] - uv[0], dy = C.uv[S + i] - uv[1];
  const float e2 = dx * dx + dy * dy;
  return e2 < C.err[i];
}

__device__ __forceinline__ Pose load_pose(const Grp& g) {
  Pose P;
#pragma unroll
  for (int k = 0; k < 9; ++k) P.R[k] = g.R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) P.t[k] = g.t[k];
  return P;
}

__device__ inline bool kept(uint8_t en) { return (en & 1) && !(en & 2) && !(en & 4); }

__device__ __forceinline__ void pose_to_tcw(const Pose& P, float* T) {   // Rcw / tcw converted to CV_32F inside an identity
  identity16(T);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[r * 4 + c] = (float)P.R[r * 3 + c];
    T[r * 4 + 3] = (float)P.t[r];
  }
}

__device__ __forceinline__ void solve(MpShared& sh, const Corr& C, int p, int n, int cap, const morb_mlpnp_solver_params& prm, const Camera& cam,
                                      const uint8_t* __restrict__ d_entry, const float* __restrict__ d_uv, const float* __restrict__ d_sigma2,
                                      const float* __restrict__ d_Xw, int nIterations, const int* __restrict__ d_rand, int randCap,
                                      morb_mlpnp_solver_state* __restrict__ d_state, uint8_t* d_best, uint8_t* __restrict__ d_inliers,
                                      int* __restrict__ d_hyp, int hypCap) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, gi = t / MP_GL, gl = t % MP_GL;
  const size_t pc = (size_t)p * cap;
  const int S = C.stride;
  // ---- the constructor: compaction in feature order ----
  for (int base = 0; base < n; base += MP_NT) {
    const int i = base + t;
    const bool valid = i < n && kept(d_entry[pc + i]);
    const int c = ordered_slot(valid, lane, wv, sh.wcount, &sh.nc);
    if (valid) {
      const float u = d_uv[(pc + i) * 2], v = d_uv[(pc + i) * 2 + 1];
      float ray[3];
      morbcam::unproject(cam, u, v, ray);
      C.br[c] = ray[0] / ray[2]; C.br[S + c] = ray[1] / ray[2];   // cv_br /= cv_br.z: not a unit vector
#pragma unroll
      for (int r = 0; r < 3; ++r) C.X[r * S + c] = d_Xw[(pc + i) * 3 + r];
      C.uv[c] = u; C.uv[S + c] = v;
      C.err[c] = morbpnp::mlpnp_max_error(d_sigma2[pc + i], prm.th2);
      C.id[c] = i;
    }
    ordered_commit<MP_NW>(sh.wcount, &sh.nc);
  }
  const int N = sh.N;
  const int minInl = morbpnp::mlpnp_min_inliers(N, prm.minInliers, prm.minSet, prm.epsilon);
  const int budget = ransac_budget(N, minInl, morbpnp::mlpnp_epsilon(N, minInl, prm.epsilon), prm.probability, prm.maxIterations);
  const int it0 = d_state[p].iterations;
  const int minSet = prm.minSet;
  if (t == 0) {
    sh.iters = it0;
    sh.bestInliers = d_state[p].bestInliers;
    sh.improved = 0; sh.done = 0; sh.refFail = 0;
  }
  if (N < minInl) {   // iterate's early return (:106-110)
    if (t == 0) {
      morb_mlpnp_solver_state& st = d_state[p];
      st.N = N; st.minInliers = minInl; st.budget = budget; st.ok = 0; st.noMore = 1; st.nInliers = 0; st.refined = 0; st.returnedAt = -1;
      identity16(st.Tcw);
    }
    return;
  }
  int end = morbpnp::mlpnp_call_end(it0, budget, nIterations);
  if (randCap / minSet < end) end = max(randCap / minSet, it0);
  __syncthreads();
  Pose refinedPose;
  for (int b0 = it0; b0 < end && !sh.done; b0 += MP_G) {
    const int nb = min(MP_G, end - b0);
    if (gi < nb) {   // one row of 16 lanes per hypothesis: sampling (RandomInt + swap with back) and computePose
      Grp& g = sh.grp[gi];
      if (gl == 0) {
        const int* r = d_rand + (size_t)p * randCap + (size_t)minSet * (size_t)(b0 + gi);
        for (int i = 0; i < minSet; ++i) {
          const int size = N - i;
          const int randi = random_int(r[i], size);
          int v = randi, bv = size - 1;
          for (int k = 0; k < i; ++k) {   // the latest substitution of a position wins
            if (g.pos[k] == randi) v = g.val[k];
            if (g.pos[k] == size - 1) bv = g.val[k];
          }
          g.idx[i] = v;
          g.pos[i] = randi; g.val[i] = bv;
        }
      }
      MORB_ROW_SYNC();
      g_compute_pose(g, C, g.idx, minSet, gl);
    }
    __syncthreads();
    for (int h0 = 0; h0 < nb; h0 += MP_NW) {   // CheckInliers, one wave per hypothesis
      const int h = h0 + wv;
      if (h < nb) {
        const Pose P = load_pose(sh.grp[h]);
        int cnt = 0;
        for (int base = 0; base < N; base += 64) {
          const int i = base + lane;
          const bool in = i < N && is_inlier(C, i, P, cam);
          cnt += __popcll(__ballot(in));
        }
        if (lane == 0) sh.cnt[h] = cnt;
      }
    }
    __syncthreads();
    for (int h = 0; h < nb; ++h) {   // the bookkeeping of iterate (:166-202), in iteration order
      const int g = b0 + h, c = sh.cnt[h];
      const int bestBefore = sh.bestInliers;
      const bool tried = sh.refFail != 0;
      __syncthreads();
      if (t == 0) {
        sh.iters = g + 1;
        if (d_hyp && g < hypCap) d_hyp[(size_t)p * hypCap + g] = c;
      }
      if (c < minInl) continue;
      if (c > bestBefore) {   // mvbBestInliers = mvbInliersi, mnBestInliers, mBestTcw
        const Pose P = load_pose(sh.grp[h]);
        for (int i = t; i < N; i += MP_NT) d_best[pc + C.id[i]] = is_inlier(C, i, P, cam) ? 1 : 0;
        if (t == 0) {
          float T[16];
          pose_to_tcw(P, T);
          for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 4; ++k) sh.bestTcw[r * 4 + k] = T[r * 4 + k];
          sh.bestInliers = c;
          sh.improved = 1;
          sh.refFail = 0;
        }
        __syncthreads();
      } else if (tried) {
        continue;   // Refine() of an unchanged best mask fails as it did before
      }
      // ---- Refine() (:295-353): computePose over the best inliers, then CheckInliers ----
      if (t == 0) sh.nList = 0;
      __syncthreads();
      for (int base = 0; base < N; base += MP_NT) {
        const int i = base + t;
        const bool valid = i < N && d_best[pc + C.id[i]] != 0;
        const int c = ordered_slot(valid, lane, wv, sh.wcount, &sh.nList);
        if (valid) C.list[c] = i;
        ordered_commit<MP_NW>(sh.wcount, &sh.nList);
      }
      if (gi == 0) g_compute_pose(sh.grp[0], C, C.list, sh.nList, gl);
      if (t == 0) sh.nRef = 0;
      __syncthreads();
      refinedPose = load_pose(sh.grp[0]);
      int cnt = 0;
      for (int base = 0; base < N; base += MP_NT) {
        const int i = base + t;
        cnt += __popcll(__ballot(i < N && is_inlier(C, i, refinedPose, cam)));
      }
      if (lane == 0) atomicAdd(&sh.nRef, cnt);
      __syncthreads();
      if (t == 0) {
        if (sh.nRef > minInl) sh.done = 1;
        else sh.refFail = 1;
      }
      __syncthreads();
      if (sh.done) break;
    }
    __syncthreads();
  }
  // ---- what iterate returns ----
  const bool refined = sh.done != 0;
  const int iters = sh.iters, best = sh.bestInliers;
  const bool spent = iters >= budget;
  const bool viaBest = !refined && spent && best >= minInl;
  if (refined) {
    for (int i = t; i < N; i += MP_NT)
      if (is_inlier(C, i, refinedPose, cam)) d_inliers[pc + C.id[i]] = 1;
  } else if (viaBest) {
    for (int i = t; i < N; i += MP_NT)
      if (d_best[pc + C.id[i]]) d_inliers[pc + C.id[i]] = 1;
  }
  if (t == 0) {
    morb_mlpnp_solver_state& st = d_state[p];
    st.N = N; st.minInliers = minInl; st.budget = budget;
    st.iterations = iters;
    st.bestInliers = best;
    st.ok = refined || viaBest;
    st.noMore = !refined && spent;
    st.nInliers = refined ? sh.nRef : (viaBest ? best : 0);
    st.refined = refined;
    st.returnedAt = refined ? iters - 1 : -1;
    if (sh.improved) {
      identity16(st.bestTcw);
      for (int k = 0; k < 12; ++k) st.bestTcw[k] = sh.bestTcw[k];
    }
    if (refined) pose_to_tcw(refinedPose, st.Tcw);
    else if (viaBest) { for (int k = 0; k < 16; ++k) st.Tcw[k] = st.bestTcw[k]; }
    else identity16(st.Tcw);
  }
}

__global__ __launch_bounds__(MP_NT) void k_mlpnp_solver(int cap, const morb_mlpnp_solver_params* __restrict__ d_params,
                                                        const uint8_t* __restrict__ d_entry, const float* __restrict__ d_uv,
                                                        const float* __restrict__ d_sigma2, const float* __restrict__ d_Xw, int nIterations,
                                                        const int* __restrict__ d_rand, int randCap,
                                                        morb_mlpnp_solver_state* __restrict__ d_state, uint8_t* d_best,
                                                        uint8_t* __restrict__ d_inliers, int* __restrict__ d_hyp, int hypCap,
                                                        char* __restrict__ ws, size_t wsPitch) {
  __shared__ MpShared sh;
  const int p = blockIdx.x, t = threadIdx.x;
  const morb_mlpnp_solver_params prm = d_params[p];
  const int n = min(max(prm.n, 0), cap);
  const size_t pc = (size_t)p * cap;
  if (prm.minSet < 6 || prm.minSet > MP_MAXSET) {   // the entry point cannot see a device-side field: no iteration, budget 0 marks it
    for (int i = t; i < cap; i += MP_NT) d_inliers[pc + i] = 0;
    if (t == 0) {
      morb_mlpnp_solver_state& st = d_state[p];
      st.N = 0; st.minInliers = prm.minInliers; st.budget = 0; st.ok = 0; st.noMore = 1; st.nInliers = 0; st.refined = 0; st.returnedAt = -1;
      identity16(st.Tcw);
    }
    return;
  }
  Camera cam;
  cam.kb8 = prm.cam[0] != 0.f;
  for (int i = 0; i < 8; ++i) cam.p[i] = prm.cam[1 + i];
  // vbInliers = vector<bool>(size, false); mvbBestInliers is empty until an iteration reaches minInliers
  const bool firstBest = d_state[p].bestInliers == 0;
  for (int i = t; i < cap; i += MP_NT) {
    d_inliers[pc + i] = 0;
    if (firstBest) d_best[pc + i] = 0;
  }
  if (t == 0) { sh.N = 0; sh.nc = 0; }
  __syncthreads();
  block_count<MP_NT>(n, &sh.N, [=](int i) { return kept(d_entry[pc + i]); });
  // two inlined call sites: in the first the correspondence arrays are known to be LDS, so it addresses them with ds_* instructions
  if (sh.N <= MP_LDS_N)
    solve(sh, mp_carve(sh.corr, MP_LDS_N), p, n, cap, prm, cam, d_entry, d_uv, d_sigma2, d_Xw, nIterations, d_rand, randCap, d_state, d_best,
          d_inliers, d_hyp, hypCap);
  else
    solve(sh, mp_carve((float*)(ws + (size_t)p * wsPitch), cap), p, n, cap, prm, cam, d_entry, d_uv, d_sigma2, d_Xw, nIterations, d_rand,
          randCap, d_state, d_best, d_inliers, d_hyp, hypCap);
}

}  // namespace

extern "C" int morb_mlpnp_solver_batch(morb_optimizer* o, int nprob, int cap, const morb_mlpnp_solver_params* d_params, const uint8_t* d_entry,
                                       const float* d_uv, const float* d_sigma2, const float* d_Xw, int nIterations, const int* d_rand,
                                       int randCap, morb_mlpnp_solver_state* d_state, uint8_t* d_bestInliers, uint8_t* d_inliers,
                                       int* d_hypInliers, int hypCap, void* stream) {
  MORB_REQUIRE(o && d_params && d_entry && d_uv && d_sigma2 && d_Xw && d_state && d_bestInliers && d_inliers, MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nprob > 0 && cap > 0 && randCap >= 0 && (d_rand || randCap == 0) && (d_hypInliers == nullptr || hypCap >= 0),
               MORB_ERR_INVALID, "bad sizes");
  MORB_ENTER(st, o, stream);
  size_t pitch;
  char* ws;
  const int rc = morb::grow_beyond_lds(o->mlpnpCorr, nprob, cap, MP_LDS_N, MP_W, &ws, &pitch);
  if (rc != MORB_OK) return rc;
  hipLaunchKernelGGL(k_mlpnp_solver, dim3(nprob), dim3(MP_NT), 0, st, cap, d_params, d_entry, d_uv, d_sigma2, d_Xw, nIterations, d_rand,
                     randCap, d_state, d_bestInliers, d_inliers, d_hypInliers, hypCap, ws, pitch);
  MORB_HIP_CHECK(hipGetLastError());
  return MORB_OK;
}
