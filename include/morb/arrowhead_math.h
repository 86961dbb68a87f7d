// The arrowhead system of Optimizer::InertialOptimization, solved as such: plain C++ that compiles for the host and for the device,
// written once (the kernel in csrc/inertial_optimization.hip runs these steps on lanes, tests/native/arrowhead_check.cc serially).
//
//   [ T + lambda I   B            ] [ x ]   [ r  ]      T: block-tridiagonal, N diagonal 3 x 3 blocks T_k (one keyframe velocity each) and
//   [ B^T            C + lambda I ] [ g ] = [ rg ]         sub-diagonal blocks O_k = T(k, k-1), O_0 unused; B: N blocks of 3 x NG; C: NG x NG.
//
// Block LDL^T down the chain, T + lambda I = L D L^T with L(k, k-1) = O_k D_{k-1}^-1:
//   D_k = T_k + lambda I - O_k D_{k-1}^-1 O_k^T,         F'_k = F_k - O_k D_{k-1}^-1 F'_{k-1}      (F = [B | r], NG + 1 columns)
// then the Schur complement  S = C + lambda I - sum_k F'_B,k^T D_k^-1 F'_B,k,  rg' = rg - sum_k F'_B,k^T D_k^-1 f'_r,k,  S g = rg',
// then up the chain          x_k = D_k^-1 (f'_r,k - F'_B,k g - O_{k+1}^T x_{k+1}).
// A zero O_k (a broken chain) is no special case.  Every pivot must be positive: a step that meets one that is not (a NaN is not) reports
// failure and the caller takes its rejected-step path.  All 3 x 3 blocks are row-major.
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define MORB_ARROW_FN __host__ __device__ __forceinline__
#define MORB_ARROW_UNROLL _Pragma("unroll")
#else
#define MORB_ARROW_FN inline
#define MORB_ARROW_UNROLL
#endif

namespace morbarrow {

constexpr int NG = 9;        // border width: gyro bias 3, accelerometer bias 3, gravity direction 2, scale 1
constexpr int NF = NG + 1;   // carried columns: the border and the right-hand side

// inverse of a symmetric positive definite 3 x 3 through its LDL^T (the lower triangle of A is read); false when a pivot is not positive
MORB_ARROW_FN bool spd3_inverse(const double* A, double* Ainv) {
  const double d0 = A[0];
  if (!(d0 > 0)) return false;
  const double l10 = A[3] / d0, l20 = A[6] / d0;
  const double d1 = A[4] - l10 * A[3];
  if (!(d1 > 0)) return false;
  const double u21 = A[7] - l20 * A[3];
  const double l21 = u21 / d1;
  const double d2 = A[8] - l20 * A[6] - l21 * u21;
  if (!(d2 > 0)) return false;
  // A^-1 = L^-T D^-1 L^-1 with L^-1 = [1 0 0; -l10 1 0; l10 l21 - l20, -l21, 1]
  const double m20 = l10 * l21 - l20;
  const double i0 = 1.0 / d0, i1 = 1.0 / d1, i2 = 1.0 / d2;
  Ainv[0] = i0 + l10 * l10 * i1 + m20 * m20 * i2;
  Ainv[1] = Ainv[3] = -l10 * i1 - m20 * l21 * i2;
  Ainv[2] = Ainv[6] = m20 * i2;
  Ainv[4] = i1 + l21 * l21 * i2;
  Ainv[5] = Ainv[7] = -l21 * i2;
  Ainv[8] = i2;
  return true;
}

// M = O Dprev^-1 (3 x 3), the multiplier block of step k; step 0 has none
MORB_ARROW_FN void chain_multiplier(const double* O, const double* DinvPrev, double* M) {
  MORB_ARROW_UNROLL
  for (int r = 0; r < 3; ++r)
    MORB_ARROW_UNROLL
    for (int c = 0; c < 3; ++c) M[r * 3 + c] = O[r * 3] * DinvPrev[c] + O[r * 3 + 1] * DinvPrev[3 + c] + O[r * 3 + 2] * DinvPrev[6 + c];
}

// D_k^-1 from T_k, lambda and (first == false) the multiplier M = O_k D_{k-1}^-1 with O_k; false when D_k is not positive definite
MORB_ARROW_FN bool chain_pivot(const double* T, double lambda, bool first, const double* M, const double* O, double* Dinv) {
  double D[9];
  MORB_ARROW_UNROLL
  for (int r = 0; r < 3; ++r)
    MORB_ARROW_UNROLL
    for (int c = 0; c <= r; ++c) {
      double v = T[r * 3 + c] + (r == c ? lambda : 0.0);
      if (!first) v -= M[r * 3] * O[c * 3] + M[r * 3 + 1] * O[c * 3 + 1] + M[r * 3 + 2] * O[c * 3 + 2];
      D[r * 3 + c] = v;
    }
  return spd3_inverse(D, Dinv);
}

// one carried column through step k: f' = f - M f'_prev (in place in `prev`, which becomes this step's column)
MORB_ARROW_FN void chain_forward_column(const double* f, bool first, const double* M, double* prev) {
  double o[3];
  MORB_ARROW_UNROLL
  for (int r = 0; r < 3; ++r) o[r] = first ? f[r] : f[r] - (M[r * 3] * prev[0] + M[r * 3 + 1] * prev[1] + M[r * 3 + 2] * prev[2]);
  prev[0] = o[0]; prev[1] = o[1]; prev[2] = o[2];
}

// the term of keyframe k in entry (i, j) of the Schur sum: F'_k[:, i]^T D_k^-1 F'_k[:, j]; Fp = the 3 x NF block of carried columns, row-major
MORB_ARROW_FN double schur_term(const double* Fp, const double* Dinv, int i, int j) {
  const double a0 = Fp[i], a1 = Fp[NF + i], a2 = Fp[2 * NF + i];
  const double b0 = Fp[j], b1 = Fp[NF + j], b2 = Fp[2 * NF + j];
  return a0 * (Dinv[0] * b0 + Dinv[1] * b1 + Dinv[2] * b2) + a1 * (Dinv[3] * b0 + Dinv[4] * b1 + Dinv[5] * b2) +
         a2 * (Dinv[6] * b0 + Dinv[7] * b1 + Dinv[8] * b2);
}

// y_k = f'_r,k - F'_B,k g: the part of the back-substitution that does not wait for the chain
MORB_ARROW_FN void back_rhs(const double* Fp, const double* g, double* y) {
  MORB_ARROW_UNROLL
  for (int r = 0; r < 3; ++r) {
    double s = Fp[r * NF + NG];
    for (int c = 0; c < NG; ++c) s -= Fp[r * NF + c] * g[c];
    y[r] = s;
  }
}

// x_k = D_k^-1 (y_k - O_{k+1}^T x_{k+1}); last == true for k = N - 1
MORB_ARROW_FN void chain_back(const double* Dinv, const double* y, bool last, const double* Onext, const double* xnext, double* x) {
  double t[3];
  MORB_ARROW_UNROLL
  for (int r = 0; r < 3; ++r) t[r] = last ? y[r] : y[r] - (Onext[r] * xnext[0] + Onext[3 + r] * xnext[1] + Onext[6 + r] * xnext[2]);
  MORB_ARROW_UNROLL
  for (int r = 0; r < 3; ++r) x[r] = Dinv[r * 3] * t[0] + Dinv[r * 3 + 1] * t[1] + Dinv[r * 3 + 2] * t[2];
}

// S g = rhs for the NG x NG corner by LDL^T in place (S row-major, lower triangle read and overwritten); false when a pivot is not positive,
// g then untouched.  (Loops of constant extent: on the device the substitution vector stays in registers.)
MORB_ARROW_FN bool corner_solve(double* S, const double* rhs, double* g) {
  double y[NG];
  for (int j = 0; j < NG; ++j) {
    const double d = S[j * NG + j];
    if (!(d > 0)) return false;
    for (int r = NG - 1; r > j; --r) {   // descending rows: S[c][j] for c < r is still the un-scaled column entry
      const double l = S[r * NG + j] / d;
      for (int c = j + 1; c <= r; ++c) S[r * NG + c] -= l * S[c * NG + j];
      S[r * NG + j] = l;
    }
  }
  MORB_ARROW_UNROLL
  for (int r = 0; r < NG; ++r) {
    double s = rhs[r];
    MORB_ARROW_UNROLL
    for (int c = 0; c < NG; ++c) if (c < r) s -= S[r * NG + c] * y[c];
    y[r] = s;
  }
  MORB_ARROW_UNROLL
  for (int r = 0; r < NG; ++r) y[r] /= S[r * NG + r];
  MORB_ARROW_UNROLL
  for (int r = NG - 1; r >= 0; --r) {
    double s = y[r];
    MORB_ARROW_UNROLL
    for (int c = 0; c < NG; ++c) if (c > r) s -= S[c * NG + r] * y[c];
    y[r] = s;
  }
  MORB_ARROW_UNROLL
  for (int r = 0; r < NG; ++r) g[r] = y[r];
  return true;
}

// The whole solve, one step after the other (what the kernel spreads over lanes).  T, O, Dinv: N x 9; F: N x 3 x NF = [B | r] (kept);
// Fp: N x 3 x NF workspace; C: NG x NG; x: N x 3; g: NG.  false = not positive definite.
inline bool solve_serial(int N, const double* T, const double* O, const double* F, const double* C, const double* rg, double lambda,
                         double* Dinv, double* Fp, double* x, double* g) {
  double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, col[NF][3];
  for (int k = 0; k < N; ++k) {
    const bool first = k == 0;
    if (!first) chain_multiplier(O + 9 * k, Dinv + 9 * (k - 1), M);
    if (!chain_pivot(T + 9 * k, lambda, first, M, O + 9 * k, Dinv + 9 * k)) return false;
    for (int c = 0; c < NF; ++c) {
      const double f[3] = {F[(k * 3 + 0) * NF + c], F[(k * 3 + 1) * NF + c], F[(k * 3 + 2) * NF + c]};
      chain_forward_column(f, first, M, col[c]);
      for (int r = 0; r < 3; ++r) Fp[(k * 3 + r) * NF + c] = col[c][r];
    }
  }
  double S[NG * NG], rhs[NG];
  for (int i = 0; i < NG; ++i) {
    for (int j = 0; j <= i; ++j) {
      double s = 0;
      for (int k = 0; k < N; ++k) s += schur_term(Fp + (size_t)k * 3 * NF, Dinv + 9 * k, i, j);
      S[i * NG + j] = C[i * NG + j] + (i == j ? lambda : 0.0) - s;
    }
    double s = 0;
    for (int k = 0; k < N; ++k) s += schur_term(Fp + (size_t)k * 3 * NF, Dinv + 9 * k, i, NG);
    rhs[i] = rg[i] - s;
  }
  if (!corner_solve(S, rhs, g)) return false;
  for (int k = N - 1; k >= 0; --k) {
    double y[3];
    back_rhs(Fp + (size_t)k * 3 * NF, g, y);
    const bool last = k == N - 1;
    chain_back(Dinv + 9 * k, y, last, last ? nullptr : O + 9 * (k + 1), last ? nullptr : x + 3 * (k + 1), x + 3 * k);
  }
  return true;
}

}  // namespace morbarrow
