// TwoViewReconstruction (reference src/TwoViewReconstruction.cc, GeometricTools::Triangulate of src/GeometricTools.cc:48-72, called by
// Pinhole::ReconstructWithTwoViews, src/CameraModels/Pinhole.cpp:85-98) for MI355X (gfx950), batched: one 256-thread workgroup per
// problem (two frames of the keypoint pool and the vnMatches12 row morb_search_for_initialization_batch wrote).  Each problem restates
//   * Reconstruct (:41-130): mvMatches12 compacted in frame-1 order (ransac_block.h), the sets of eight by DUtils::Random::RandomInt and
//     swap-with-back on the caller's rand() values (include/morb/two_view_math.h), the choice by RH > 0.50;
//   * Normalize (:723-768) over ALL keypoints of each frame, FindHomography / FindFundamental (:132-225), ComputeH21 / ComputeF21
//     (:227-303), CheckHomography / CheckFundamental (:305-471), ReconstructF / DecomposeE (:473-560, :882-905), ReconstructH
//     (:562-721), CheckRT (:770-880) and Triangulate, every float expression in the reference's order (-ffp-contract=off).
// Mapping.  The matches (u1 v1 u2 v2, frame-1 index, flags, cosParallax: TV_W words) live in LDS up to TV_LDS_N, in the handle's
// twoViewCorr workspace beyond.  Iterations run TV_ROUND at a time: a row of 16 lanes per iteration builds both hypotheses (A^T A in
// FP64 in LDS, lane k owning row / column k of a Jacobi rotation: row_jacobi.h), then one LANE per hypothesis walks all N matches and adds its score
// terms one after the other, so the float sum is the reference's sequential sum bit for bit (waves 0-1 score H, waves 2-3 F); the
// running best is then taken in iteration order with the strict >.  The four sums of Normalize are chains as well: the workgroup
// stages one keypoint per thread at a time in LDS and one lane per sum adds them in index order.  CheckRT runs one match per thread (the
// 4 x 4 null vector in registers); vCosParallax is not sorted: the element at min(50, size - 1) is found by counting, per element,
// how many are smaller (ties by match index).
// Decisions taken here ("TwoViewReconstruction"):
//   * Eigen's JacobiSVD is replaced by the project's own routines: the null vector of A (8 x 9, 16 x 9, 4 x 4) is the eigenvector of
//     the first smallest |eigenvalue| of A^T A, formed and solved in FP64 by one cyclic Jacobi (the float one loses the last singular
//     vector) and rounded to float; a 3 x 3 SVD is built on the same Jacobi (V and w from M^T M by decreasing eigenvalue, u0 and u1 from
//     M v, u2 = u0 x u1, v2 = v0 x v1, w2 signed like det M; ReconstructH moves that sign into V).  The sign of a singular vector is
//     therefore ours: CheckHomography / CheckFundamental do not see it, in ReconstructH it permutes the eight hypotheses.
//   * the score sums and the Normalize sums are sequential (above); only the terms are computed in parallel.
//   * acos on a float is glibc 2.35's acosf (libm_f32.h).
//   * fewer than 8 matches (undefined in the reference): no iteration, ok = 0, model = 0.
//   * Triangulate returning false (x3Dh(3) == 0) leaves CheckRT's point unset in the reference; here the match is skipped, as a
//     non-finite point is.
//   * ReconstructH never assigns vP3D in this fork (:712-718; upstream does): here the winning hypothesis' points are returned on
//     both paths.
//   * a vnMatches12 entry >= the second frame's count is read as no match (the reference would read beyond mvKeys2).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "handles.h"
#include "libm_f32.h"
#include "morb_hip.h"
#include "morb/two_view_math.h"
#include "ransac_block.h"
#include "row_jacobi.h"

#ifndef MORB_TWO_VIEW_THREADS
#define MORB_TWO_VIEW_THREADS 256
#endif

namespace {

using namespace morbtv;
using namespace morbransac;

constexpr int TV_NT = MORB_TWO_VIEW_THREADS;
constexpr int TV_NW = TV_NT / 64;
constexpr int TV_GL = morbrow::ROW_LANES;   // lanes per hypothesis row
constexpr int TV_G = TV_NT / TV_GL;     // rows
constexpr int TV_ROUND = TV_NT / 2;     // iterations per round: one scoring lane per (iteration, model)
constexpr int TV_LDS_N = 512;           // matches held in LDS; beyond, the global workspace
constexpr int TV_W = 7;                 // words per match
constexpr int TV_CHUNK = TV_NT;         // keypoints staged per step of Normalize, one per thread
// 128 and 256 are the shapes built and measured; 512 would need 92 KB of LDS
static_assert(TV_NT == 128 || TV_NT == 256, "two scoring halves of whole waves, TvShared within 64 KB");

struct Corr {   // structure of arrays, `stride` entries each
  float *u1, *v1, *u2, *v2, *cs;
  int *i1, *fl;   // fl: bit 0 inlier of the chosen model, bit 1 counted by the current CheckRT
  int stride;
};
__device__ inline Corr tv_carve(float* base, int stride) {
  Corr c;
  c.u1 = base; c.v1 = base + stride; c.u2 = base + 2 * stride; c.v2 = base + 3 * stride; c.cs = base + 4 * stride;
  c.i1 = (int*)(base + 5 * stride); c.fl = (int*)(base + 6 * stride);
  c.stride = stride;
  return c;
}

struct Grp {   // the LDS of one 16-lane row
  double W[162];   // A = W (9 x 9, row-major), V = W + 81
  double red[TV_GL];
  float pn[32];    // the eight normalised sample points: x1 y1 x2 y2 each
};

struct TvShared {
  float corr[TV_LDS_N * TV_W];
  Grp grp[TV_G];
  union {
    float chunk[4][TV_CHUNK];    // Normalize: x1 y1 x2 y2 (then their absolute deviations) of the staged keypoints
    float hyp[TV_ROUND][27];     // per iteration of the round: H21i, H12i, F21i
  };
  float score[2][TV_ROUND];
  float nrm[8];                  // meanX1 meanY1 meanX2 meanY2, then sX1 sY1 sX2 sY2
  float best[27];                // the best H21, its H12, the best F21
  float SH, SF, sel;
  int bestIt[2];
  float R[8][9], t[8][3], par[8];
  int nGood[8];
  int wcount[TV_NW];
  int N, nc, cnt, nhyp;
};

// ---- small float matrices (row-major), every product summed k = 0, 1, 2 left to right --------------------------------------------
__device__ __forceinline__ void mul33(const float* A, const float* B, float* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
__device__ __forceinline__ void transpose33(const float* A, float* T) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) T[i * 3 + j] = A[j * 3 + i];
}
__device__ __forceinline__ float det33(const float* a) {
  return a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
}
__device__ __forceinline__ void inverse33(const float* a, float* o) {   // the adjugate times 1 / det
  const float inv = 1.0f / det33(a);
  o[0] = (a[4] * a[8] - a[5] * a[7]) * inv; o[1] = (a[2] * a[7] - a[1] * a[8]) * inv; o[2] = (a[1] * a[5] - a[2] * a[4]) * inv;
  o[3] = (a[5] * a[6] - a[3] * a[8]) * inv; o[4] = (a[0] * a[8] - a[2] * a[6]) * inv; o[5] = (a[2] * a[3] - a[0] * a[5]) * inv;
  o[6] = (a[3] * a[7] - a[4] * a[6]) * inv; o[7] = (a[1] * a[6] - a[0] * a[7]) * inv; o[8] = (a[0] * a[4] - a[1] * a[3]) * inv;
}

// ---- cyclic Jacobi of a symmetric M x M matrix in registers (one thread): v receives the eigenvectors as columns ----------------------
template <int M>
__device__ __forceinline__ void jacobi_reg(double* a, double* v) {
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) v[i * M + j] = i == j ? 1.0 : 0.0;
  double fro = 0;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    double c = 0;
#pragma unroll
    for (int i = 0; i < M; ++i) c += a[i * M + j] * a[i * M + j];
    fro += c;
  }
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double c = 0;
#pragma unroll
      for (int i = 0; i < M; ++i)
        if (i < j) c += a[i * M + j] * a[i * M + j];
      off += c;
    }
    if (!(off > 1e-30 * fro)) break;
#pragma unroll
    for (int p = 0; p < M - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < M; ++q) {
        const double apq = a[p * M + q];
        if (apq != 0.0) {
          const double app = a[p * M + p], aqq = a[q * M + q];
          const double theta = (aqq - app) / (2.0 * apq);
          const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
          for (int k = 0; k < M; ++k) {
            if (k != p && k != q) {
              const double akp = a[k * M + p], akq = a[k * M + q];
              const double np_ = c * akp - s * akq, nq = s * akp + c * akq;
              a[k * M + p] = np_; a[p * M + k] = np_;
              a[k * M + q] = nq; a[q * M + k] = nq;
            }
            const double vkp = v[k * M + p], vkq = v[k * M + q];
            v[k * M + p] = c * vkp - s * vkq;
            v[k * M + q] = s * vkp + c * vkq;
          }
          a[p * M + p] = app - t * apq;
          a[q * M + q] = aqq + t * apq;
          a[p * M + q] = 0.0;
          a[q * M + p] = 0.0;
        }
      }
  }
}

// M = U diag(w) V^T of a float 3 x 3 (header comment): one thread
__device__ __forceinline__ void svd3(const float* M, float* U, float* w, float* Vo) {
  double Md[9], B[9], V[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) Md[i] = (double)M[i];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) B[i * 3 + j] = Md[i] * Md[j] + Md[3 + i] * Md[3 + j] + Md[6 + i] * Md[6 + j];
  jacobi_reg<3>(B, V);
  int o0 = 0, o1 = 1, o2 = 2;
  double l0 = B[0], l1 = B[4], l2 = B[8];
  if (l1 > l0) { const double tv = l0; l0 = l1; l1 = tv; const int ti = o0; o0 = o1; o1 = ti; }
  if (l2 > l1) { const double tv = l1; l1 = l2; l2 = tv; const int ti = o1; o1 = o2; o2 = ti; }
  if (l1 > l0) { const double tv = l0; l0 = l1; l1 = tv; const int ti = o0; o0 = o1; o1 = ti; }
  double v0[3], v1[3], v2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    v0[i] = o0 == 0 ? V[i * 3] : (o0 == 1 ? V[i * 3 + 1] : V[i * 3 + 2]);
    v1[i] = o1 == 0 ? V[i * 3] : (o1 == 1 ? V[i * 3 + 1] : V[i * 3 + 2]);
  }
  double a0[3], a1[3], u0[3], u1[3], u2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    a0[i] = Md[i * 3] * v0[0] + Md[i * 3 + 1] * v0[1] + Md[i * 3 + 2] * v0[2];
    a1[i] = Md[i * 3] * v1[0] + Md[i * 3 + 1] * v1[1] + Md[i * 3 + 2] * v1[2];
  }
  const double n0 = sqrt(a0[0] * a0[0] + a0[1] * a0[1] + a0[2] * a0[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) u0[i] = a0[i] / n0;
  const double d = u0[0] * a1[0] + u0[1] * a1[1] + u0[2] * a1[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) a1[i] = a1[i] - d * u0[i];
  const double n1 = sqrt(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) u1[i] = a1[i] / n1;
  u2[0] = u0[1] * u1[2] - u0[2] * u1[1];
  u2[1] = u0[2] * u1[0] - u0[0] * u1[2];
  u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
  v2[0] = v0[1] * v1[2] - v0[2] * v1[1];
  v2[1] = v0[2] * v1[0] - v0[0] * v1[2];
  v2[2] = v0[0] * v1[1] - v0[1] * v1[0];
  double a2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) a2[i] = Md[i * 3] * v2[0] + Md[i * 3 + 1] * v2[1] + Md[i * 3 + 2] * v2[2];
  const bool neg = u2[0] * a2[0] + u2[1] * a2[1] + u2[2] * a2[2] < 0;   // det M < 0
  w[0] = (float)sqrt(l0 < 0 ? 0.0 : l0);
  w[1] = (float)sqrt(l1 < 0 ? 0.0 : l1);
  w[2] = (float)sqrt(l2 < 0 ? 0.0 : l2);
  if (neg) w[2] = -w[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    U[i * 3] = (float)u0[i]; U[i * 3 + 1] = (float)u1[i]; U[i * 3 + 2] = (float)u2[i];
    Vo[i * 3] = (float)v0[i]; Vo[i * 3 + 1] = (float)v1[i]; Vo[i * 3 + 2] = (float)v2[i];
  }
}

// ---- the 9 x 9 Jacobi of one 16-lane row (row_jacobi.h: the arithmetic of jacobi_reg, lane k owning row / column k) ------------------
// the eigenvector of the first smallest |eigenvalue|, rounded to float; every lane of the row returns it
__device__ __forceinline__ void g_null9(Grp& g, int l, float* x) {
  morbrow::g_jacobi(g.W, g.W + 81, g.red, 9, l);
  int kmin = 0;
  double best = fabs(g.W[0]);
  for (int k = 1; k < 9; ++k) {
    const double v = fabs(g.W[k * 9 + k]);
    if (v < best) { best = v; kmin = k; }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) x[k] = (float)g.W[81 + k * 9 + kmin];
  MORB_ROW_SYNC();
}
// lane l (< 9) adds column l of A^T A: acc[i] += a[i] * a[l] for one row a of A
__device__ __forceinline__ void ata_row(const float* a, int l, double* acc) {
  float al = 0.f;
#pragma unroll
  for (int c = 0; c < 9; ++c) al = (c == l) ? a[c] : al;
#pragma unroll
  for (int i = 0; i < 9; ++i) acc[i] += (double)a[i] * (double)al;
}

// ComputeH21 (:227-265) and ComputeF21 (:267-303) of the eight points in g.pn, de-normalised (:166-167, :215): out = H21i, H12i, F21i
__device__ __forceinline__ void g_hypotheses(Grp& g, int l, const float* T1, const float* T2inv, const float* T2t, float* out) {
  double acc[9];
  float x[9], tmp[9];
  // ---- H ----
#pragma unroll
  for (int i = 0; i < 9; ++i) acc[i] = 0.0;
  for (int p = 0; p < 8; ++p) {
    const float u1 = g.pn[p * 4], v1 = g.pn[p * 4 + 1], u2 = g.pn[p * 4 + 2], v2 = g.pn[p * 4 + 3];
    const float r0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2};
    const float r1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, -u2 * u1, -u2 * v1, -u2};
    ata_row(r0, l, acc);
    ata_row(r1, l, acc);
  }
  if (l < 9) {
#pragma unroll
    for (int i = 0; i < 9; ++i) g.W[i * 9 + l] = acc[i];
  }
  MORB_ROW_SYNC();
  g_null9(g, l, x);
  mul33(T2inv, x, tmp);
  mul33(tmp, T1, out);
  inverse33(out, out + 9);
  // ---- F ----
#pragma unroll
  for (int i = 0; i < 9; ++i) acc[i] = 0.0;
  for (int p = 0; p < 8; ++p) {
    const float u1 = g.pn[p * 4], v1 = g.pn[p * 4 + 1], u2 = g.pn[p * 4 + 2], v2 = g.pn[p * 4 + 3];
    const float r0[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f};
    ata_row(r0, l, acc);
  }
  if (l < 9) {
#pragma unroll
    for (int i = 0; i < 9; ++i) g.W[i * 9 + l] = acc[i];
  }
  MORB_ROW_SYNC();
  g_null9(g, l, x);
  float U[9], w[3], V[9], Fn[9];
  svd3(x, U, w, V);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Fn[i * 3 + j] = (U[i * 3] * w[0]) * V[j * 3] + (U[i * 3 + 1] * w[1]) * V[j * 3 + 1];
  mul33(T2t, Fn, tmp);
  mul33(tmp, T1, out + 18);
}

// one match of CheckHomography (:339-388): adds its terms to score in the reference's order, returns bIn
__device__ __forceinline__ bool h_match(const float* H21, const float* H12, float u1, float v1, float u2, float v2, float invSigmaSquare,
                                        float& score) {
  const float th = 5.991f;
  bool bIn = true;
  const float w2in1inv = 1.0f / (H12[6] * u2 + H12[7] * v2 + H12[8]);
  const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
  const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
  const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > th) bIn = false;
  else score += th - chiSquare1;
  const float w1in2inv = 1.0f / (H21[6] * u1 + H21[7] * v1 + H21[8]);
  const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
  const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
  const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > th) bIn = false;
  else score += th - chiSquare2;
  return bIn;
}
// one match of CheckFundamental (:417-468)
__device__ __forceinline__ bool f_match(const float* F, float u1, float v1, float u2, float v2, float invSigmaSquare, float& score) {
  const float th = 3.841f, thScore = 5.991f;
  bool bIn = true;
  const float a2 = F[0] * u1 + F[1] * v1 + F[2];
  const float b2 = F[3] * u1 + F[4] * v1 + F[5];
  const float c2 = F[6] * u1 + F[7] * v1 + F[8];
  const float num2 = a2 * u2 + b2 * v2 + c2;
  const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > th) bIn = false;
  else score += thScore - chiSquare1;
  const float a1 = F[0] * u2 + F[3] * v2 + F[6];
  const float b1 = F[1] * u2 + F[4] * v2 + F[7];
  const float c1 = F[2] * u2 + F[5] * v2 + F[8];
  const float num1 = a1 * u1 + b1 * v1 + c1;
  const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > th) bIn = false;
  else score += thScore - chiSquare2;
  return bIn;
}

__device__ __forceinline__ bool finitef(float x) { return (morbm::f2u(x) & 0x7f800000u) != 0x7f800000u; }

struct RtCtx { float K[9], R[9], t[3], P1[12], P2[12], O2[3], th2; };
__device__ __forceinline__ void rt_setup(RtCtx& c, const float* K, const float* R, const float* t, float th2) {
  float Rt[12];
#pragma unroll
  for (int i = 0; i < 9; ++i) { c.K[i] = K[i]; c.R[i] = R[i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) c.t[i] = t[i];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) { c.P1[i * 4 + j] = j < 3 ? K[i * 3 + j] : 0.f; Rt[i * 4 + j] = j < 3 ? R[i * 3 + j] : t[i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) c.P2[i * 4 + j] = K[i * 3] * Rt[j] + K[i * 3 + 1] * Rt[4 + j] + K[i * 3 + 2] * Rt[8 + j];
#pragma unroll
  for (int i = 0; i < 3; ++i) c.O2[i] = (-R[i]) * t[0] + (-R[3 + i]) * t[1] + (-R[6 + i]) * t[2];
  c.th2 = th2;
}
// one inlier match of CheckRT (:806-869): true when it is counted (nGood); p = the point, cosParallax, low = cosParallax < 0.99998
__device__ __forceinline__ bool rt_match(const RtCtx& c, float x1, float y1, float x2, float y2, float* p, float& cosParallax, bool& low) {
  float A[16];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    A[j] = x1 * c.P1[8 + j] - c.P1[j];
    A[4 + j] = y1 * c.P1[8 + j] - c.P1[4 + j];
    A[8 + j] = x2 * c.P2[8 + j] - c.P2[j];
    A[12 + j] = y2 * c.P2[8 + j] - c.P2[4 + j];
  }
  double B[16], V[16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) s += (double)A[r * 4 + i] * (double)A[r * 4 + j];
      B[i * 4 + j] = s;
    }
  jacobi_reg<4>(B, V);
  int kmin = 0;
  double best = fabs(B[0]);
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const double v = fabs(B[k * 4 + k]);
    if (v < best) { best = v; kmin = k; }
  }
  float h[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) h[k] = (float)(kmin == 0 ? V[k * 4] : (kmin == 1 ? V[k * 4 + 1] : (kmin == 2 ? V[k * 4 + 2] : V[k * 4 + 3])));
  if (h[3] == 0) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = h[k] / h[3];
  if (!finitef(p[0]) || !finitef(p[1]) || !finitef(p[2])) return false;
  const float dist1 = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  const float n2[3] = {p[0] - c.O2[0], p[1] - c.O2[1], p[2] - c.O2[2]};
  const float dist2 = sqrtf(n2[0] * n2[0] + n2[1] * n2[1] + n2[2] * n2[2]);
  cosParallax = (p[0] * n2[0] + p[1] * n2[1] + p[2] * n2[2]) / (dist1 * dist2);
  low = (double)cosParallax < 0.99998;
  if (p[2] <= 0 && low) return false;
  float q[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) q[r] = c.R[r * 3] * p[0] + c.R[r * 3 + 1] * p[1] + c.R[r * 3 + 2] * p[2] + c.t[r];
  if (q[2] <= 0 && low) return false;
  const float fx = c.K[0], fy = c.K[4], cx = c.K[2], cy = c.K[5];
  const float invZ1 = 1.0f / p[2];
  const float im1x = fx * p[0] * invZ1 + cx, im1y = fy * p[1] * invZ1 + cy;
  const float squareError1 = (im1x - x1) * (im1x - x1) + (im1y - y1) * (im1y - y1);
  if (squareError1 > c.th2) return false;
  const float invZ2 = 1.0f / q[2];
  const float im2x = fx * q[0] * invZ2 + cx, im2y = fy * q[1] * invZ2 + cy;
  const float squareError2 = (im2x - x2) * (im2x - x2) + (im2y - y2) * (im2y - y2);
  if (squareError2 > c.th2) return false;
  return true;
}

// DecomposeE (:882-905) and the four hypotheses of ReconstructF (:499-506): one thread
__device__ __forceinline__ void decompose_f(TvShared& sh, const float* K, const float* F) {
  float Kt[9], tmp[9], E[9], U[9], V[9], Vt[9], w[3];
  transpose33(K, Kt);
  mul33(Kt, F, tmp);
  mul33(tmp, K, E);
  svd3(E, U, w, V);
  transpose33(V, Vt);
  float t[3] = {U[2], U[5], U[8]};
  const float tn = sqrtf(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = t[k] / tn;
  const float W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
  float Wt[9], R1[9], R2[9];
  transpose33(W, Wt);
  mul33(U, W, tmp);
  mul33(tmp, Vt, R1);
  if (det33(R1) < 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R1[i] = -R1[i];
  }
  mul33(U, Wt, tmp);
  mul33(tmp, Vt, R2);
  if (det33(R2) < 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R2[i] = -R2[i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int k = 0; k < 9; ++k) sh.R[i][k] = (i & 1) ? R2[k] : R1[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) sh.t[i][k] = i < 2 ? t[k] : -t[k];
  }
  sh.nhyp = 4;
}

// the eight hypotheses of ReconstructH (:574-680): one thread; false on the d1 / d2, d2 / d3 test (:590)
__device__ __forceinline__ bool decompose_h(TvShared& sh, const float* K, const float* H21) {
  float invK[9], tmp[9], A[9], U[9], V[9], Vt[9], w[3];
  inverse33(K, invK);
  mul33(invK, H21, tmp);
  mul33(tmp, K, A);
  svd3(A, U, w, V);
  if (w[2] < 0) { w[2] = -w[2]; V[2] = -V[2]; V[5] = -V[5]; V[8] = -V[8]; }
  transpose33(V, Vt);
  const float s = det33(U) * det33(Vt);
  const float d1 = w[0], d2 = w[1], d3 = w[2];
  if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;
  const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
  const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
  const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
  const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
  const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
  float sU[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) sU[i] = s * U[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = i & 3;
    const float x1 = j < 2 ? aux1 : -aux1;                 // {aux1, aux1, -aux1, -aux1}
    const float x3 = (j & 1) ? -aux3 : aux3;               // {aux3, -aux3, aux3, -aux3}
    const bool pos = j == 0 || j == 3;                     // stheta / sphi = {aux, -aux, -aux, aux}
    float Rp[9], tp[3];
    if (i < 4) {
      const float st = pos ? aux_stheta : -aux_stheta;
      Rp[0] = ctheta; Rp[1] = 0.f; Rp[2] = -st; Rp[3] = 0.f; Rp[4] = 1.f; Rp[5] = 0.f; Rp[6] = st; Rp[7] = 0.f; Rp[8] = ctheta;
      tp[0] = x1; tp[1] = 0.f; tp[2] = -x3;
#pragma unroll
      for (int k = 0; k < 3; ++k) tp[k] *= d1 - d3;
    } else {
      const float sp = pos ? aux_sphi : -aux_sphi;
      Rp[0] = cphi; Rp[1] = 0.f; Rp[2] = sp; Rp[3] = 0.f; Rp[4] = -1.f; Rp[5] = 0.f; Rp[6] = sp; Rp[7] = 0.f; Rp[8] = -cphi;
      tp[0] = x1; tp[1] = 0.f; tp[2] = x3;
#pragma unroll
      for (int k = 0; k < 3; ++k) tp[k] *= d1 + d3;
    }
    float R[9], tt[3];
    mul33(sU, Rp, tmp);
    mul33(tmp, Vt, R);
#pragma unroll
    for (int k = 0; k < 3; ++k) tt[k] = U[k * 3] * tp[0] + U[k * 3 + 1] * tp[1] + U[k * 3 + 2] * tp[2];
    const float n = sqrtf(tt[0] * tt[0] + tt[1] * tt[1] + tt[2] * tt[2]);
#pragma unroll
    for (int k = 0; k < 9; ++k) sh.R[i][k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) sh.t[i][k] = tt[k] / n;
  }
  sh.nhyp = 8;
  return true;
}

struct Args {
  int cap, maxIterations, randCap;
  const int *img1, *img2, *count, *matches12, *rnd;
  const morb_keypoint* kps;
  const float *K4, *sigma;
  int *ok, *stats;
  float *T21, *P3D, *fstats, *hypScores;
  uint8_t *tri, *inlH, *inlF;
};

// CheckRT (:770-880) of hypothesis h over the chosen mask: nGood and parallax to sh; with `emit`, vP3D / vbGood of the counted matches
__device__ __forceinline__ void check_rt(TvShared& sh, const Corr& C, int N, const float* K, float th2, int h, bool emit, float* P3D, uint8_t* tri) {
  const int t = threadIdx.x, lane = t & 63;
  RtCtx c;
  rt_setup(c, K, sh.R[h], sh.t[h], th2);
  if (t == 0) { sh.cnt = 0; sh.sel = 0.f; }
  __syncthreads();
  int cnt = 0;
  for (int base = 0; base < N; base += TV_NT) {
    const int i = base + t;
    bool good = false;
    if (i < N && (C.fl[i] & 1)) {
      float p[3], cs = 0.f;
      bool low = false;
      good = rt_match(c, C.u1[i], C.v1[i], C.u2[i], C.v2[i], p, cs, low);
      if (good) {
        C.cs[i] = cs;
        if (emit) {
          const size_t o = (size_t)C.i1[i];
          P3D[o * 3] = p[0]; P3D[o * 3 + 1] = p[1]; P3D[o * 3 + 2] = p[2];
          if (low) tri[o] = 1;
        }
      }
    }
    if (i < N) C.fl[i] = (C.fl[i] & 1) | (good ? 2 : 0);
    cnt += __popcll(__ballot(good));
  }
  if (lane == 0) atomicAdd(&sh.cnt, cnt);
  __syncthreads();
  const int nGood = sh.cnt;
  if (emit) return;
  if (nGood > 0) {   // the element at min(50, size - 1) of the sorted list, by counting the smaller ones
    const int idx = nGood - 1 < TV_PARALLAX_RANK ? nGood - 1 : TV_PARALLAX_RANK;
    for (int i = t; i < N; i += TV_NT) {
      if (!(C.fl[i] & 2)) continue;
      const float v = C.cs[i];
      int rank = 0;
      for (int j = 0; j < N; ++j) {
        if (!(C.fl[j] & 2)) continue;
        const float u = C.cs[j];
        rank += (u < v || (u == v && j < i)) ? 1 : 0;
      }
      if (rank == idx) sh.sel = v;
    }
  }
  __syncthreads();
  if (t == 0) {
    sh.nGood[h] = nGood;
    sh.par[h] = nGood > 0 ? tv_parallax_deg(morbm::acosf_glibc(sh.sel)) : 0.f;
  }
  __syncthreads();
}

__device__ __forceinline__ void solve(TvShared& sh, const Corr& C, int p, const Args& a, int n1, int n2, const morb_keypoint* k1,
                                      const morb_keypoint* k2) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, gi = t / TV_GL, gl = t % TV_GL;
  const size_t pc = (size_t)p * a.cap;
  const int N = sh.N;
  const int maxIt = a.maxIterations;
  // ---- mvMatches12 in frame-1 order (:55-64) ----
  for (int base = 0; base < n1; base += TV_NT) {
    const int i = base + t;
    int m = -1;
    if (i < n1) m = a.matches12[pc + i];
    const bool valid = m >= 0 && m < n2;
    const int c = ordered_slot(valid, lane, wv, sh.wcount, &sh.nc);
    if (valid) {
      C.u1[c] = k1[i].x; C.v1[c] = k1[i].y; C.u2[c] = k2[m].x; C.v2[c] = k2[m].y;
      C.i1[c] = i; C.fl[c] = 0;
    }
    ordered_commit<TV_NW>(sh.wcount, &sh.nc);
  }
  // ---- Normalize (:723-768): the four sums of each pass are chains over all keypoints in index order ----
  for (int pass = 0; pass < 2; ++pass) {
    float acc = 0.f;
    const int nmax = n1 > n2 ? n1 : n2;
    for (int base = 0; base < nmax; base += TV_CHUNK) {
      const int i = base + t;
      {
        float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
        if (i < n1) { x1 = k1[i].x; y1 = k1[i].y; }
        if (i < n2) { x2 = k2[i].x; y2 = k2[i].y; }
        if (pass == 1) {
          x1 = morbm::fabsf_(x1 - sh.nrm[0]); y1 = morbm::fabsf_(y1 - sh.nrm[1]);
          x2 = morbm::fabsf_(x2 - sh.nrm[2]); y2 = morbm::fabsf_(y2 - sh.nrm[3]);
        }
        sh.chunk[0][t] = x1; sh.chunk[1][t] = y1; sh.chunk[2][t] = x2; sh.chunk[3][t] = y2;
      }
      __syncthreads();
      if (t < 4) {
        const int n = t < 2 ? n1 : n2;
        const int cnt = n - base < TV_CHUNK ? n - base : TV_CHUNK;
        for (int k = 0; k < cnt; ++k) acc += sh.chunk[t][k];
      }
      __syncthreads();
    }
    if (t < 4) {
      const int n = t < 2 ? n1 : n2;
      const float mean = acc / n;
      sh.nrm[pass * 4 + t] = pass == 0 ? mean : 1.0f / mean;
    }
    __syncthreads();
  }
  const float mX1 = sh.nrm[0], mY1 = sh.nrm[1], mX2 = sh.nrm[2], mY2 = sh.nrm[3];
  const float sX1 = sh.nrm[4], sY1 = sh.nrm[5], sX2 = sh.nrm[6], sY2 = sh.nrm[7];
  const float T1[9] = {sX1, 0.f, -mX1 * sX1, 0.f, sY1, -mY1 * sY1, 0.f, 0.f, 1.f};
  const float T2[9] = {sX2, 0.f, -mX2 * sX2, 0.f, sY2, -mY2 * sY2, 0.f, 0.f, 1.f};
  float T2inv[9], T2t[9];
  inverse33(T2, T2inv);
  transpose33(T2, T2t);
  const float sigma = a.sigma[p];
  const float invSigmaSquare = 1.0f / (sigma * sigma);
  if (t == 0) { sh.SH = 0.f; sh.SF = 0.f; sh.bestIt[0] = -1; sh.bestIt[1] = -1; }
  if (t < 27) sh.best[t] = 0.f;
  __syncthreads();
  // ---- FindHomography / FindFundamental (:132-225), TV_ROUND iterations at a time ----
  const int* rnd = a.rnd + (size_t)p * a.randCap;
  for (int r0 = 0; r0 < maxIt; r0 += TV_ROUND) {
    const int nb = maxIt - r0 < TV_ROUND ? maxIt - r0 : TV_ROUND;
    for (int s0 = 0; s0 < nb; s0 += TV_G) {
      const int slot = s0 + gi;
      if (slot < nb) {
        Grp& g = sh.grp[gi];
        if (gl == 0) {
          int idx[TV_SET];
          tv_sample8(rnd + (size_t)TV_SET * (size_t)(r0 + slot), N, idx);
#pragma unroll
          for (int j = 0; j < TV_SET; ++j) {
            const int c = idx[j] < N ? idx[j] : N - 1;   // (a value outside [0, 2^31) is not a rand() value: stay inside the arrays)
            g.pn[j * 4] = (C.u1[c] - mX1) * sX1; g.pn[j * 4 + 1] = (C.v1[c] - mY1) * sY1;
            g.pn[j * 4 + 2] = (C.u2[c] - mX2) * sX2; g.pn[j * 4 + 3] = (C.v2[c] - mY2) * sY2;
          }
        }
        MORB_ROW_SYNC();
        float out[27];
        g_hypotheses(g, gl, T1, T2inv, T2t, out);
        if (gl == 0) {
#pragma unroll
          for (int k = 0; k < 27; ++k) sh.hyp[slot][k] = out[k];
        }
      }
    }
    __syncthreads();
    {   // one lane per (iteration, model): the score is the reference's sequential float sum
      const int model = t / TV_ROUND, slot = t % TV_ROUND;
      if (slot < nb) {
        float M[18];
        float score = 0.f;
        if (model == 0) {
#pragma unroll
          for (int k = 0; k < 18; ++k) M[k] = sh.hyp[slot][k];
          for (int i = 0; i < N; ++i) h_match(M, M + 9, C.u1[i], C.v1[i], C.u2[i], C.v2[i], invSigmaSquare, score);
        } else {
#pragma unroll
          for (int k = 0; k < 9; ++k) M[k] = sh.hyp[slot][18 + k];
          for (int i = 0; i < N; ++i) f_match(M, C.u1[i], C.v1[i], C.u2[i], C.v2[i], invSigmaSquare, score);
        }
        sh.score[model][slot] = score;
        if (a.hypScores) a.hypScores[((size_t)p * 2 + model) * maxIt + r0 + slot] = score;
      }
    }
    __syncthreads();
    if (t == 0) {   // if (currentScore > score), in iteration order (:171-175, :219-223)
      for (int h = 0; h < nb; ++h) {
        if (sh.score[0][h] > sh.SH) {
          sh.SH = sh.score[0][h]; sh.bestIt[0] = r0 + h;
          for (int k = 0; k < 18; ++k) sh.best[k] = sh.hyp[h][k];
        }
        if (sh.score[1][h] > sh.SF) {
          sh.SF = sh.score[1][h]; sh.bestIt[1] = r0 + h;
          for (int k = 0; k < 9; ++k) sh.best[18 + k] = sh.hyp[h][18 + k];
        }
      }
    }
    __syncthreads();
  }
  // ---- the choice (:111-129) ----
  const float SH = sh.SH, SF = sh.SF;
  const bool none = SH + SF == 0.f;
  const float RH = none ? 0.f : SH / (SH + SF);
  const int model = none ? 0 : (RH > 0.50 ? 1 : 2);
  float Mb[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) Mb[k] = sh.best[k];
  if (t == 0) sh.cnt = 0;
  __syncthreads();
  {   // vbMatchesInliersH / F of the kept iterations; the chosen model's goes to the flags
    int cnt = 0;
    for (int base = 0; base < N; base += TV_NT) {
      const int i = base + t;
      bool inH = false, inF = false, in = false;
      if (i < N) {
        float dummy = 0.f;
        if (sh.bestIt[0] >= 0) inH = h_match(Mb, Mb + 9, C.u1[i], C.v1[i], C.u2[i], C.v2[i], invSigmaSquare, dummy);
        if (sh.bestIt[1] >= 0) inF = f_match(Mb + 18, C.u1[i], C.v1[i], C.u2[i], C.v2[i], invSigmaSquare, dummy);
        if (a.inlH) a.inlH[pc + i] = inH;
        if (a.inlF) a.inlF[pc + i] = inF;
        in = model == 1 ? inH : (model == 2 ? inF : false);
        C.fl[i] = in ? 1 : 0;
      }
      cnt += __popcll(__ballot(in));
    }
    if (lane == 0) atomicAdd(&sh.cnt, cnt);
  }
  __syncthreads();
  const int nIn = sh.cnt;
  __syncthreads();
  const float K[9] = {a.K4[p * 4], 0.f, a.K4[p * 4 + 2], 0.f, a.K4[p * 4 + 1], a.K4[p * 4 + 3], 0.f, 0.f, 1.f};
  const float th2 = (float)(4.0 * (double)(sigma * sigma));
  int fail = TV_FAIL_NONE, chosen = -1;
  if (t == 0) {
    sh.nhyp = 0;
    for (int h = 0; h < 8; ++h) { sh.nGood[h] = 0; sh.par[h] = 0.f; }
    if (model == 1) decompose_h(sh, K, Mb);
    else if (model == 2) decompose_f(sh, K, Mb + 18);
  }
  __syncthreads();
  const int nhyp = sh.nhyp;
  for (int h = 0; h < nhyp; ++h) check_rt(sh, C, N, K, th2, h, false, nullptr, nullptr);
  if (model == 0) fail = TV_FAIL_ZERO_SCORE;
  else if (model == 1 && nhyp == 0) fail = TV_FAIL_DEGENERATE_H;
  else if (model == 1) {   // :682-720
    int bestGood = 0, secondBestGood = 0, bestIdx = -1;
    float bestParallax = -1.f;
    for (int h = 0; h < 8; ++h) {
      const int g = sh.nGood[h];
      if (g > bestGood) { secondBestGood = bestGood; bestGood = g; bestIdx = h; bestParallax = sh.par[h]; }
      else if (g > secondBestGood) secondBestGood = g;
    }
    const bool counts = (double)secondBestGood < 0.75 * (double)bestGood && bestGood > TV_MIN_TRIANGULATED && (double)bestGood > 0.9 * (double)nIn;
    if (counts && bestParallax >= TV_MIN_PARALLAX) chosen = bestIdx;
    else fail = counts ? TV_FAIL_PARALLAX : TV_FAIL_AMBIGUOUS;
  } else {   // :508-559
    int maxGood = sh.nGood[0];
    for (int h = 1; h < 4; ++h) maxGood = sh.nGood[h] > maxGood ? sh.nGood[h] : maxGood;
    const int nMinGood = tv_min_good(nIn, TV_MIN_TRIANGULATED);
    int nsimilar = 0;
    for (int h = 0; h < 4; ++h) nsimilar += ((double)sh.nGood[h] > 0.7 * (double)maxGood) ? 1 : 0;
    if (maxGood < nMinGood || nsimilar > 1) fail = TV_FAIL_AMBIGUOUS;
    else {
      int first = 0;
      while (sh.nGood[first] != maxGood) ++first;
      if (sh.par[first] > TV_MIN_PARALLAX) chosen = first;
      else fail = TV_FAIL_PARALLAX;
    }
  }
  if (chosen >= 0) check_rt(sh, C, N, K, th2, chosen, true, a.P3D + pc * 3, a.tri + pc);
  if (t == 0) {
    int* st = a.stats + (size_t)p * TV_STATS_LEN;
    float* fs = a.fstats + (size_t)p * TV_FSTATS_LEN;
    st[TV_S_N] = N; st[TV_S_MODEL] = model; st[TV_S_BEST_IT_H] = sh.bestIt[0]; st[TV_S_BEST_IT_F] = sh.bestIt[1];
    st[TV_S_NINLIERS] = nIn; st[TV_S_NHYP] = nhyp; st[TV_S_CHOSEN] = chosen; st[TV_S_FAIL] = fail;
    for (int h = 0; h < 8; ++h) { st[TV_S_NGOOD0 + h] = sh.nGood[h]; fs[TV_F_PARALLAX0 + h] = sh.par[h]; }
    fs[TV_F_SH] = SH; fs[TV_F_SF] = SF; fs[TV_F_RH] = RH;
    for (int k = 0; k < 9; ++k) { fs[TV_F_H21_0 + k] = Mb[k]; fs[TV_F_F21_0 + k] = Mb[18 + k]; }
    a.ok[p] = chosen >= 0;
    if (chosen >= 0) {
      for (int k = 0; k < 9; ++k) a.T21[(size_t)p * 12 + k] = sh.R[chosen][k];
      for (int k = 0; k < 3; ++k) a.T21[(size_t)p * 12 + 9 + k] = sh.t[chosen][k];
    }
  }
}

__global__ __launch_bounds__(TV_NT) void k_two_view(Args a, char* __restrict__ ws, size_t wsPitch) {
  __shared__ TvShared sh;
  const int p = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const int cap = a.cap;
  const size_t pc = (size_t)p * cap;
  const int n1 = min(max(a.count[a.img1[p]], 0), cap), n2 = min(max(a.count[a.img2[p]], 0), cap);
  const morb_keypoint* k1 = a.kps + (size_t)a.img1[p] * cap;
  const morb_keypoint* k2 = a.kps + (size_t)a.img2[p] * cap;
  // what the reference leaves unwritten is zero: vP3D / vbTriangulated beyond the winner's points, both masks, the rows of a problem
  // that runs no iteration
  for (int i = t; i < cap; i += TV_NT) {
    a.P3D[(pc + i) * 3] = 0.f; a.P3D[(pc + i) * 3 + 1] = 0.f; a.P3D[(pc + i) * 3 + 2] = 0.f;
    a.tri[pc + i] = 0;
    if (a.inlH) a.inlH[pc + i] = 0;
    if (a.inlF) a.inlF[pc + i] = 0;
  }
  if (a.hypScores)
    for (int i = t; i < 2 * a.maxIterations; i += TV_NT) a.hypScores[(size_t)p * 2 * a.maxIterations + i] = 0.f;
  if (t < 12) a.T21[(size_t)p * 12 + t] = 0.f;
  if (t == 0) { sh.N = 0; sh.nc = 0; }
  __syncthreads();
  int cnt = 0;   // (block_count of ransac_block.h, written out: the test of m sits outside the guard of the load here)
  for (int base = 0; base < n1; base += TV_NT) {
    const int i = base + t;
    int m = -1;
    if (i < n1) m = a.matches12[pc + i];
    cnt += __popcll(__ballot(m >= 0 && m < n2));
  }
  if (lane == 0) atomicAdd(&sh.N, cnt);
  __syncthreads();
  const int N = sh.N;
  if (N < TV_SET) {   // no iteration
    if (t < TV_STATS_LEN) a.stats[(size_t)p * TV_STATS_LEN + t] = t == TV_S_N ? N : (t == TV_S_BEST_IT_H || t == TV_S_BEST_IT_F || t == TV_S_CHOSEN ? -1 : (t == TV_S_FAIL ? TV_FAIL_FEW_MATCHES : 0));
    if (t < TV_FSTATS_LEN) a.fstats[(size_t)p * TV_FSTATS_LEN + t] = 0.f;
    if (t == 0) a.ok[p] = 0;
    return;
  }
  // two inlined call sites: in the first the match arrays are known to be LDS, so it addresses them with ds_* instructions
  if (N <= TV_LDS_N) solve(sh, tv_carve(sh.corr, TV_LDS_N), p, a, n1, n2, k1, k2);
  else solve(sh, tv_carve((float*)(ws + (size_t)p * wsPitch), cap), p, a, n1, n2, k1, k2);
}

}  // namespace

extern "C" int morb_two_view_reconstruction_batch(morb_optimizer* o, int nprob, int cap, const int* d_img1, const int* d_img2, const int* d_count,
                                                  const morb_keypoint* d_kpsUn, const int* d_matches12, const float* d_K4, const float* d_sigma,
                                                  int maxIterations, const int* d_rand, int randCap, int* d_ok, float* d_T21, float* d_P3D,
                                                  uint8_t* d_triangulated, int* d_stats, float* d_fstats, uint8_t* d_inliersH, uint8_t* d_inliersF,
                                                  float* d_hypScores, void* stream) {
  MORB_REQUIRE(o && d_img1 && d_img2 && d_count && d_kpsUn && d_matches12 && d_K4 && d_sigma && d_rand && d_ok && d_T21 && d_P3D &&
                   d_triangulated && d_stats && d_fstats, MORB_ERR_INVALID, "NULL argument");
  MORB_REQUIRE(nprob > 0 && cap >= 1, MORB_ERR_INVALID, "bad sizes");
  MORB_REQUIRE(maxIterations >= 1, MORB_ERR_INVALID, "maxIterations < 1");
  MORB_REQUIRE((long long)randCap >= 8ll * (long long)maxIterations, MORB_ERR_INVALID, "randCap < 8 * maxIterations");
  MORB_ENTER(st, o, stream);
  size_t pitch;
  char* ws;
  const int rc = morb::grow_beyond_lds(o->twoViewCorr, nprob, cap, TV_LDS_N, TV_W, &ws, &pitch);
  if (rc != MORB_OK) return rc;
  Args a;
  a.cap = cap; a.maxIterations = maxIterations; a.randCap = randCap;
  a.img1 = d_img1; a.img2 = d_img2; a.count = d_count; a.matches12 = d_matches12; a.rnd = d_rand;
  a.kps = d_kpsUn; a.K4 = d_K4; a.sigma = d_sigma;
  a.ok = d_ok; a.stats = d_stats; a.T21 = d_T21; a.P3D = d_P3D; a.fstats = d_fstats; a.hypScores = d_hypScores;
  a.tri = d_triangulated; a.inlH = d_inliersH; a.inlF = d_inliersF;
  hipLaunchKernelGGL(k_two_view, dim3(nprob), dim3(TV_NT), 0, st, a, ws, pitch);
  MORB_HIP_CHECK(hipGetLastError());
  return MORB_OK;
}
