// Test-only probe of the dense FP64 building blocks: morbdense::ldlt_solve / ldlt_solve_global (dense_ldlt.h) and
// morbschur::k_schur_mfma + schur_sum4 (schur_mfma.h), each launched ALONE with the sizes and limits the product launches them with
// (local_ba.hip: k_g_ldlt_lds / k_g_ldlt_global / k_g_schur_finish, inertial_ba.hip: k_iba_solve_lds / k_iba_solve_blocked).
// Built by morb_slam_amd/build.py: build_test_native() with the library's own flags into tests/native/libdense_probe.so; it is not part of
// libmorb_hip.so.  Nothing here allocates device memory: every buffer is the caller's (a torch tensor's data_ptr()).  Every launch is on
// the null stream and is waited for; the return value is 0, a HIP error code, or one of the negative refusals below (nothing launched).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "ba_host.h"
#include "dense_ldlt.h"
#include "schur_mfma.h"

namespace {

constexpr int PROBE_ERR_SIZE = -1;   // n out of the solver's range
constexpr int PROBE_ERR_LDS = -2;    // the dynamic LDS the solver needs is beyond the product's limit
constexpr int PROBE_ERR_ARG = -3;    // a null buffer

template <bool PIVOT_POSITIVE>
__global__ __launch_bounds__(morbdense::LT) void k_probe_ldlt_lds(const double* H, const double* b, double* x, int n, int* okOut) {
  extern __shared__ double sLd[];
  __shared__ int sOk;
  const bool ok = morbdense::ldlt_solve<PIVOT_POSITIVE>(H, b, x, n, sLd, &sOk);
  if (threadIdx.x == 0) *okOut = ok ? 1 : 0;
}

template <bool PIVOT_POSITIVE>
__global__ __launch_bounds__(morbdense::GT) void k_probe_ldlt_global(double* A, const double* b, double* x, int n, double* pnlG, int panelInLds,
                                                                     int* okOut) {
  extern __shared__ double sLd[];   // dblk | y | (the panel copies when they fit)
  __shared__ int sOk;
  double* pnl = panelInLds ? sLd + morbdense::global_lds_doubles(n) : pnlG;
  const bool ok = morbdense::ldlt_solve_global<PIVOT_POSITIVE>(A, b, x, n, pnl, sLd, &sOk);
  if (threadIdx.x == 0) *okOut = ok ? 1 : 0;
}

// C[r][c] (r <= c < ncols) from the partial products, four lanes per element, every lane of every wave calls schur_sum4
// (k_g_schur_finish's mapping: a lane beyond the matrix sums element (0, 0) and writes nothing)
__global__ __launch_bounds__(256) void k_probe_schur_sum(const double* __restrict__ part, const int* __restrict__ blkIndex, int nb, int nblk,
                                                         int nsplit, int ncols, double* __restrict__ C) {
  const int t = blockIdx.x * 256 + threadIdx.x, gid = t >> 2, q = t & 3;
  const bool live = gid < ncols * ncols;
  const int r = live ? gid / ncols : 0, c = live ? gid - r * ncols : 0;
  const int i = r < c ? r : c, j = r < c ? c : r;
  const double cs = morbschur::schur_sum4(part, blkIndex, nb, nblk, nsplit, i, j, q);
  if (q == 0 && live && r <= c) C[(size_t)r * ncols + c] = cs;
}

int finish() {   // the launch's own error first, then whatever the kernel ran into
  hipError_t e = hipGetLastError();
  const hipError_t s = hipDeviceSynchronize();
  if (e == hipSuccess) e = s;
  return (int)e;
}

struct I2 { int x, y; };   // (int2's layout; ba_host.h is host only)

}  // namespace

extern "C" {

// out[0..5] = lds_doubles(n), global_lds_doubles(n), global_panel_doubles(n), and the three byte limits of dense_ldlt.h
int probe_sizes(int n, long long* out) {
  if (n < 1 || !out) return PROBE_ERR_SIZE;
  out[0] = (long long)morbdense::lds_doubles(n);
  out[1] = (long long)morbdense::global_lds_doubles(n);
  out[2] = (long long)morbdense::global_panel_doubles(n);
  out[3] = (long long)morbdense::LDS_SOLVER_LIMIT;
  out[4] = (long long)morbdense::GLOBAL_SOLVER_LIMIT;
  out[5] = (long long)morbdense::PERSISTENT_HS_LIMIT;
  return 0;
}

// out[0..8] = Mp, nb, nblk, Kp, ksteps, nsplit, stepsPerSplit, wElems(), partElems(); out[9] = SB, out[10] = SU
int probe_schur_plan(int ncols, int K, long long* out) {
  if (ncols < 1 || K < 1 || !out) return PROBE_ERR_SIZE;
  const morbschur::Plan p = morbschur::make_plan(ncols, K);
  out[0] = p.Mp; out[1] = p.nb; out[2] = p.nblk; out[3] = p.Kp; out[4] = p.ksteps; out[5] = p.nsplit; out[6] = p.stepsPerSplit;
  out[7] = (long long)p.wElems(); out[8] = (long long)p.partElems(); out[9] = morbschur::SB; out[10] = morbschur::SU;
  return 0;
}

// H [n][n], b [n], x [n] (b and x separate buffers), ok: one int.  One workgroup, dynamic LDS 8 lds_doubles(n), as k_g_ldlt_lds.
int probe_ldlt_lds(int pivot_positive, const double* H, const double* b, double* x, int n, int* ok) {
  if (!H || !b || !x || !ok) return PROBE_ERR_ARG;
  if (n < 1 || n > 192) return PROBE_ERR_SIZE;
  const size_t lds = sizeof(double) * morbdense::lds_doubles(n);
  if (lds > morbdense::LDS_SOLVER_LIMIT) return PROBE_ERR_LDS;
  const void* fn = pivot_positive ? reinterpret_cast<const void*>(&k_probe_ldlt_lds<true>) : reinterpret_cast<const void*>(&k_probe_ldlt_lds<false>);
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)morbdense::LDS_SOLVER_LIMIT);
  if (e != hipSuccess) return (int)e;
  if (pivot_positive) hipLaunchKernelGGL(k_probe_ldlt_lds<true>, dim3(1), dim3(morbdense::LT), lds, 0, H, b, x, n, ok);
  else hipLaunchKernelGGL(k_probe_ldlt_lds<false>, dim3(1), dim3(morbdense::LT), lds, 0, H, b, x, n, ok);
  return finish();
}

// A [n][n] (overwritten by the factors), b, x [n], pnlG: global_panel_doubles(n) doubles (used when panel_in_lds == 0), ok: one int.
// One workgroup, dynamic LDS as k_g_ldlt_global: dblk | y, plus the panel copies when panel_in_lds.
int probe_ldlt_global(int pivot_positive, double* A, const double* b, double* x, int n, int panel_in_lds, double* pnlG, int* ok) {
  if (!A || !b || !x || !ok || (!panel_in_lds && !pnlG)) return PROBE_ERR_ARG;
  if (n < 1) return PROBE_ERR_SIZE;
  const size_t lds = sizeof(double) * (morbdense::global_lds_doubles(n) + (panel_in_lds ? morbdense::global_panel_doubles(n) : 0));
  if (lds > morbdense::GLOBAL_SOLVER_LIMIT) return PROBE_ERR_LDS;
  const void* fn = pivot_positive ? reinterpret_cast<const void*>(&k_probe_ldlt_global<true>) : reinterpret_cast<const void*>(&k_probe_ldlt_global<false>);
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)morbdense::GLOBAL_SOLVER_LIMIT);
  if (e != hipSuccess) return (int)e;
  if (pivot_positive) hipLaunchKernelGGL(k_probe_ldlt_global<true>, dim3(1), dim3(morbdense::GT), lds, 0, A, b, x, n, pnlG, panel_in_lds, ok);
  else hipLaunchKernelGGL(k_probe_ldlt_global<false>, dim3(1), dim3(morbdense::GT), lds, 0, A, b, x, n, pnlG, panel_in_lds, ok);
  return finish();
}

// C = WD^T W on r <= c < ncols.  W, WD: wElems() doubles, zero but for the caller's [K][ncols] values at pitch Mp; part: partElems()
// doubles; blocks: 2 nblk ints and blkIndex: nb nb ints, both filled here (morb::schur_block_lists); C: [ncols][ncols], only r <= c written.
int probe_schur(int ncols, int K, const double* W, const double* WD, double* part, int* blocks, int* blkIndex, double* C, long long* plan_out) {
  if (!W || !WD || !part || !blocks || !blkIndex || !C || !plan_out) return PROBE_ERR_ARG;
  if (probe_schur_plan(ncols, K, plan_out) != 0) return PROBE_ERR_SIZE;
  const morbschur::Plan p = morbschur::make_plan(ncols, K);
  std::vector<I2> bl;
  std::vector<int> idx;
  morb::schur_block_lists(p.nb, bl, idx);
  if ((int)bl.size() != p.nblk) return PROBE_ERR_SIZE;
  hipError_t e = hipMemcpy(blocks, bl.data(), sizeof(I2) * bl.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(blkIndex, idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(morbschur::k_schur_mfma, dim3(p.nblk, p.nsplit), dim3(64), 0, 0, WD, W, p.Mp, p.ksteps, p.stepsPerSplit,
                     reinterpret_cast<const int2*>(blocks), part, (const int*)nullptr);
  const int rc = finish();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(k_probe_schur_sum, dim3((4 * ncols * ncols + 255) / 256), dim3(256), 0, 0, (const double*)part, (const int*)blkIndex, p.nb,
                     p.nblk, p.nsplit, ncols, C);
  return finish();
}

}  // extern "C"
