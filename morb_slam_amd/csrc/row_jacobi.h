// The FP64 cyclic Jacobi of a symmetric m x m matrix held in LDS, run by a row of 16 lanes (lane k owning row / column k of every
// rotation), and the wave-level synchronisation of such a row: the 12 x 12, 9 x 9 and 3 x 3 eigenproblems of mlpnp_solver.hip and
// the 9 x 9 ones of two_view.hip.  The method (pair order, skipped rotations, stopping rule) is DESIGN.md section 6, "MLPnPsolver".
#pragma once
#include <hip/hip_runtime.h>

// the 16 lanes of a row sit in one wave: their LDS writes are ordered by a wave-level fence, no workgroup barrier
#define MORB_ROW_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

namespace morbrow {

constexpr int ROW_LANES = 16;

// sum over columns j of the squares of column j's entries (all rows, or the rows above the diagonal), columns added in order;
// red: ROW_LANES doubles of the row's LDS
__device__ __forceinline__ double g_colsum(const double* A, double* red, int m, int l, bool upper) {
  double c = 0;
  if (l < m) {
    const int rows = upper ? l : m;
    for (int i = 0; i < rows; ++i) c += A[i * m + l] * A[i * m + l];
  }
  red[l] = c;
  MORB_ROW_SYNC();
  double s = 0;
  for (int j = 0; j < m; ++j) s += red[j];
  MORB_ROW_SYNC();
  return s;
}

// cyclic Jacobi of the symmetric m x m matrix A (LDS, row-major, m <= ROW_LANES) by the 16 lanes of a row; V (m x m, LDS) receives
// the eigenvectors as columns
__device__ __forceinline__ void g_jacobi(double* A, double* V, double* red, int m, int l) {
  for (int e = l; e < m * m; e += ROW_LANES) V[e] = (e / m == e % m) ? 1.0 : 0.0;
  MORB_ROW_SYNC();
  double fro = g_colsum(A, red, m, l, false);
  // The stopping rule compares sums of squares, and those leave FP64's range for entries below 1e-154 or above 1e+154: fro is then 0 or
  // inf and the loop would stop before its first rotation.  Such a matrix (never one the solvers build from image coordinates; the
  // test is one comparison of a row-uniform value) is scaled by an exact power of two first, and scaled back at the end.
  int back = 0;
  if (!(fro >= 0x1p-600 && fro <= 0x1p600)) {
    double c = 0;
    if (l < m)
      for (int i = 0; i < m; ++i) c = fmax(c, fabs(A[i * m + l]));
    red[l] = c;
    MORB_ROW_SYNC();
    double mx = 0;
    for (int j = 0; j < m; ++j) mx = fmax(mx, red[j]);
    MORB_ROW_SYNC();
    if (mx > 0 && mx < __builtin_huge_val()) {
      (void)frexp(mx, &back);
      for (int e = l; e < m * m; e += ROW_LANES) A[e] = ldexp(A[e], -back);
      MORB_ROW_SYNC();
      fro = g_colsum(A, red, m, l, false);
    }
  }
  for (int sweep = 0; sweep < 30; ++sweep) {
    const double off = g_colsum(A, red, m, l, true);
    if (!(off > 1e-30 * fro)) break;
    for (int p = 0; p < m - 1; ++p)
      for (int q = p + 1; q < m; ++q) {
        const double apq = A[p * m + q];
        if (apq == 0.0) continue;
        const double app = A[p * m + p], aqq = A[q * m + q];
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        if (l < m) {
          const int k = l;
          double np_ = 0, nq = 0;
          const bool mid = k != p && k != q;
          if (mid) {
            const double akp = A[k * m + p], akq = A[k * m + q];
            np_ = c * akp - s * akq;
            nq = s * akp + c * akq;
          }
          const double vkp = V[k * m + p], vkq = V[k * m + q];
          if (mid) {
            A[k * m + p] = np_; A[p * m + k] = np_;
            A[k * m + q] = nq; A[q * m + k] = nq;
          }
          V[k * m + p] = c * vkp - s * vkq;
          V[k * m + q] = s * vkp + c * vkq;
          if (k == p) {
            A[p * m + p] = app - t * apq;
            A[q * m + q] = aqq + t * apq;
            A[p * m + q] = 0.0;
            A[q * m + p] = 0.0;
          }
        }
        MORB_ROW_SYNC();
      }
  }
  if (back != 0) {
    for (int e = l; e < m * m; e += ROW_LANES) A[e] = ldexp(A[e], back);
    MORB_ROW_SYNC();
  }
}

}  // namespace morbrow
