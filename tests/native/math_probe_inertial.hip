// Test-only probe, the inertial_device.h family and row_jacobi.h: ExpSO3 / LogSO3 and the right Jacobians with their threshold branches,
// NormalizeRotation, the small Gauss-Jordan inverse, the eigenvalue clamp with its cyclic-Jacobi rebuild, and the row-of-16-lanes
// Jacobi of the RANSAC solvers on one wave that carries four matrices.  Part of tests/native/libmath_probe.so.
#include "math_probe_common.h"

#include "inertial_device.h"
#include "row_jacobi.h"

PROBE(exp_so3, double, 3, double, 9, exp_so3(a, o);)
PROBE(log_so3, double, 9, double, 3, log_so3(a, o);)
PROBE(right_jacobian_so3, double, 3, double, 9, right_jacobian_so3(a, o);)
PROBE(inv_right_jacobian_so3, double, 3, double, 9, inv_right_jacobian_so3(a, o);)
PROBE(normalize_rotation_f, float, 9, float, 9, for (int k = 0; k < 9; ++k) o[k] = a[k]; normalize_rotation_f(o);)

namespace {

constexpr int PROBE_DENSE_MAX_N = 16;

// thread i: A_i (n x n) -> Ainv_i, ok_i; M: 2 n n doubles of scratch per matrix.  One thread per matrix, as the product calls it.
__global__ void k_probe_invert_n(const double* A, int n, long long count, double* Ainv, double* M, int* ok) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  ok[i] = invert_n(A + i * n * n, n, Ainv + i * n * n, M + i * 2 * n * n) ? 1 : 0;
}
// thread i: S_i (n x n, in place) with the scratch matrices A_i, V_i
__global__ void k_probe_clamp(double* S, int n, double thr, long long count, double* A, double* V) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  clamp_eigenvalues(S + i * n * n, n, thr, A + i * n * n, V + i * n * n);
}

// one wave, four rows of 16 lanes, row r diagonalises matrix r: A [4][m m] in, eigenvalues W [4][m] (the diagonal left in A) and
// eigenvectors V [4][m m] out
__global__ __launch_bounds__(64) void k_probe_row_jacobi(const double* Ain, int m, double* W, double* Vout) {
  __shared__ double sA[4][morbrow::ROW_LANES * morbrow::ROW_LANES], sV[4][morbrow::ROW_LANES * morbrow::ROW_LANES], sRed[4][morbrow::ROW_LANES];
  const int row = threadIdx.x >> 4, l = threadIdx.x & 15;
  for (int e = l; e < m * m; e += morbrow::ROW_LANES) sA[row][e] = Ain[row * m * m + e];
  MORB_ROW_SYNC();
  morbrow::g_jacobi(sA[row], sV[row], sRed[row], m, l);
  MORB_ROW_SYNC();
  for (int e = l; e < m * m; e += morbrow::ROW_LANES) Vout[row * m * m + e] = sV[row][e];
  if (l < m) W[row * m + l] = sA[row][l * m + l];
}

}  // namespace

extern "C" int probe_invert_n(const double* A, int n, long long count, double* Ainv, double* M, int* ok) {
  if (!A || !Ainv || !M || !ok) return PROBE_ERR_ARG;
  if (n < 1 || n > PROBE_DENSE_MAX_N || count < 1 || count > (1 << 20)) return PROBE_ERR_SIZE;
  hipLaunchKernelGGL(k_probe_invert_n, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, 0, A, n, count, Ainv, M, ok);
  return probe_finish();
}
extern "C" int probe_clamp_eigenvalues(double* S, int n, double thr, long long count, double* A, double* V) {
  if (!S || !A || !V) return PROBE_ERR_ARG;
  if (n < 1 || n > PROBE_DENSE_MAX_N || count < 1 || count > (1 << 20)) return PROBE_ERR_SIZE;
  hipLaunchKernelGGL(k_probe_clamp, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, 0, S, n, thr, count, A, V);
  return probe_finish();
}
extern "C" int probe_row_jacobi(const double* A, int m, double* W, double* V) {
  if (!A || !W || !V) return PROBE_ERR_ARG;
  if (m < 1 || m > morbrow::ROW_LANES) return PROBE_ERR_SIZE;
  hipLaunchKernelGGL(k_probe_row_jacobi, dim3(1), dim3(64), 0, 0, A, m, W, V);
  return probe_finish();
}
