// The block LDL^T of the four whole-map graph optimisers (essential_graph.hip B = 7, pose_graph_4dof.hip 4, global_ba.hip 6,
// full_inertial_ba.hip 3): H + lambda I = L D L^T over the block ENVELOPE of envelope_plan.h, the forward substitution on the way, and the
// backward substitution.  Written once over the block size B; a unit's k_*_factor and k_*_backsub is one call with its own constants
// (k_eg_backsub excepted: Order, below).
//   * Storage.  Row i holds the B x B blocks from its first non-zero column rowFirst[i] to i, row-major, at block rowOff[i]; fill never
//     leaves the envelope.  colRows[colStart[j] .. colStart[j + 1]) are the rows below j whose envelope covers column j, ascending.  L has
//     the strictly lower blocks and unit-lower diagonal blocks; d is D.  No pivoting across blocks: a pivot that fails the unit's test
//     (POSITIVE: d > 0, as the reference's Cholesky asks; else d != 0 and not NaN) is a failed factorisation, a rejected trial.
//   * Schedule.  ONE workgroup of NT lanes takes the block columns in sequence (left-looking).  Within a column the covering rows are
//     parallel, a lane per (row, line of its block): NT / B rows take one pass, and in the usual case of one pass a line stays in its
//     lane's registers from the sums to the division.  The column's own row, scaled by D, is staged in LDS STAGE blocks at a time (a whole
//     row of any graph below that many vertices); a lane keeps PREFETCH blocks' loads of its own row in flight against it.
//   * Barriers.  Every lane factorises the B x B diagonal block for itself out of LDS instead of waiting for one lane's result: the
//     hand-round through LDS cost a barrier per column, and the column loop is nothing but latency (a few hundred columns, each a handful
//     of dependent steps).  The first stage of a column needs no barrier of its own either: it follows the last column's.  That leaves
//     three barriers per column of one pass and one stage.
//   * Order.  Per line of a block the arithmetic and its order do not depend on the schedule constants (NT, STAGE, PREFETCH): the sums
//     run over k ascending, and inside a block over p ascending, so a result is the same bits whatever the launch shape.  The 7 x 7
//     factorisation had a schedule of its own before this header (one lane factorised the diagonal block and handed it round through
//     LDS, an unconditional stage barrier) and gives the same bits on this one, 2 % faster at 500 keyframes and 0.5 % at 2000
//     (profiles/r23).  Its backward substitution does NOT use envelope_backsub: prefetching the next diagonal block into LDS is worth
//     14 to 17 % of that kernel at B = 7 (profiles/r23), so k_eg_backsub keeps its own text; at B = 4, 6 and 3 nobody has tried it.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// the envelope arrays of a unit's device record, which names them the same way
struct EnvelopeSys {
  int n;                                                // block rows
  const int *rowFirst, *rowOff, *colStart, *colRows;    // envelope_plan.h
  double *H, *L;                                        // [nBlocks][B * B] the matrix; its factor
  double *b, *y, *x, *d;                                // [B n] right-hand side, work vector, solution, D of the factorisation
};
template <class Dev>
__device__ __forceinline__ EnvelopeSys envelope_sys(const Dev& D) {
  return {D.n, D.rowFirst, D.rowOff, D.colStart, D.colRows, D.H, D.L, D.b, D.y, D.x, D.d};
}

// one line of S_ij -= L_ik (D_k L_jk^T): l = line r of L_ik, m = M_jk = L_jk D_k (row-major, in LDS)
template <int B>
__device__ __forceinline__ void envelope_line_minus(double* acc, const double* l, const double* m) {
#pragma unroll
  for (int c = 0; c < B; ++c) {
    double s = 0;
#pragma unroll
    for (int p = 0; p < B; ++p) s += l[p] * m[c * B + p];
    acc[c] -= s;
  }
}
// L_ij = S_ij L_jj^-T D_j^-1 for one line of a block below the diagonal (a: L_jj's strictly lower part); returns L_ij y_j
template <int B>
__device__ __forceinline__ double envelope_below_line(const double* s, const double (*a)[B], const double* dd, const double* yy, double* l) {
#pragma unroll
  for (int c = 0; c < B; ++c) {
    double v = s[c];
#pragma unroll
    for (int p = 0; p < c; ++p) v -= (l[p] * dd[p]) * a[c][p];
    l[c] = v / dd[c];
  }
  double dot = 0;
#pragma unroll
  for (int c = 0; c < B; ++c) dot += l[c] * yy[c];
  return dot;
}

// H + lambda I = L D L^T over the envelope, and y = L^-1 b on the way.  Called by every lane of one workgroup of NT; returns to every lane
// whether all pivots passed (after a failure L, d and y are not to be used).
template <int B, int NT, int STAGE, int PREFETCH, bool POSITIVE>
__device__ __forceinline__ bool envelope_factor(const EnvelopeSys& D, double lambda) {
  constexpr int BB = B * B;
  constexpr int PASS = NT / B * B;   // lanes at work in a pass
  static_assert(BB <= 64 && 64 + B <= NT, "lanes 0 .. BB write the diagonal block, lanes 64 .. 64 + B its d and y");
  __shared__ double sM[STAGE * BB];
  __shared__ double sS[BB];
  const int t = threadIdx.x, n = D.n;
  bool ok = true;
  for (int i = t; i < B * n; i += NT) D.y[i] = D.b[i];
  __threadfence_block();
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    const int fj = D.rowFirst[j];
    const int cs = D.colStart[j];
    const int nItems = (D.colStart[j + 1] - cs + 1) * B;   // a lane per (row, line of its block); lines 0 .. B - 1 are the diagonal block's
    const bool one = nItems <= PASS;                       // (the usual case: the lines stay in registers from the sums to the division)
    const size_t rowJ = (size_t)D.rowOff[j];
    const size_t diag = (rowJ + (j - fj)) * BB;
    double yj[B];                                          // (final since the last column's barrier)
#pragma unroll
    for (int r = 0; r < B; ++r) yj[r] = D.y[(size_t)j * B + r];
    double acc[B];
#pragma unroll
    for (int c = 0; c < B; ++c) acc[c] = 0;
    double* mine = nullptr;   // the line's place in the factor
    int myRow = 0;
    // ---- S_ij = H_ij - sum_k L_ik D_k L_jk^T, over the k both rows hold ----
    for (int base = 0; base < nItems; base += PASS) {
      const int item = base + t;
      const bool valid = t < PASS && item < nItems;
      int i = j, r = 0, fi = fj;
      size_t rowI = rowJ;
      if (valid) {
        const int w = item / B;
        r = item - w * B;
        if (w) { i = D.colRows[cs + w - 1]; fi = D.rowFirst[i]; rowI = (size_t)D.rowOff[i]; }
        const double* h = D.H + (rowI + (j - fi)) * BB + r * B;
#pragma unroll
        for (int c = 0; c < B; ++c) acc[c] = h[c] + ((i == j && c == r) ? lambda : 0.0);
        mine = D.L + (rowI + (j - fi)) * BB + r * B;
        myRow = i;
      }
      for (int c0 = fj; c0 < j; c0 += STAGE) {
        const int c1 = min(c0 + STAGE, j);
        if (base || c0 != fj) __syncthreads();   // (the column's first stage follows the last column's barrier)
        for (int q = t; q < (c1 - c0) * BB; q += NT)   // M_jk = L_jk D_k
          sM[q] = D.L[(rowJ + (c0 - fj)) * BB + q] * D.d[(size_t)(c0 + q / BB) * B + q % B];
        __syncthreads();
        if (valid) {
          const double* lik = D.L + (rowI - fi) * BB + r * B;   // + BB k: line r of L_ik
          int k = max(c0, fi);
          if constexpr (PREFETCH > 1) {
            for (; k + PREFETCH <= c1; k += PREFETCH) {   // PREFETCH blocks' loads in flight
              double l[PREFETCH][B];
#pragma unroll
              for (int u = 0; u < PREFETCH; ++u)
#pragma unroll
                for (int p = 0; p < B; ++p) l[u][p] = lik[(size_t)(k + u) * BB + p];
#pragma unroll
              for (int u = 0; u < PREFETCH; ++u) envelope_line_minus<B>(acc, l[u], sM + (k + u - c0) * BB);
            }
          }
          for (; k < c1; ++k) {
            double l[B];
#pragma unroll
            for (int p = 0; p < B; ++p) l[p] = lik[(size_t)k * BB + p];
            envelope_line_minus<B>(acc, l, sM + (k - c0) * BB);
          }
        }
      }
      if (valid) {
        if (i == j) {
#pragma unroll
          for (int c = 0; c < B; ++c) sS[r * B + c] = acc[c];
        } else if (!one) {
#pragma unroll
          for (int c = 0; c < B; ++c) mine[c] = acc[c];
        }
      }
    }
    if (!one) __threadfence_block();
    __syncthreads();
    // ---- the diagonal block, by every lane for itself: S_jj = L_jj D_j L_jj^T, and y_j = L_jj^-1 y_j ----
    double a[B][B], dd[B], yy[B];
#pragma unroll
    for (int r = 0; r < B; ++r)
#pragma unroll
      for (int c = 0; c < B; ++c) a[r][c] = c <= r ? sS[r * B + c] : 0.0;
#pragma unroll
    for (int c = 0; c < B; ++c) {
      double dc = a[c][c];
#pragma unroll
      for (int p = 0; p < c; ++p) dc -= (a[c][p] * dd[p]) * a[c][p];
      dd[c] = dc;
      if constexpr (POSITIVE) ok = ok && dc > 0;
      else ok = ok && dc != 0 && dc == dc;   // a zero or NaN pivot: the factorisation has failed
#pragma unroll
      for (int r = c + 1; r < B; ++r) {
        double v = a[r][c];
#pragma unroll
        for (int p = 0; p < c; ++p) v -= (a[r][p] * dd[p]) * a[c][p];
        a[r][c] = v / dc;
      }
    }
#pragma unroll
    for (int r = 0; r < B; ++r) {
      double v = yj[r];
#pragma unroll
      for (int p = 0; p < r; ++p) v -= a[r][p] * yy[p];
      yy[r] = v;
    }
    if (!ok) break;   // (the same for every lane)
    if (t < BB) {
      double v = 0.0;   // (written out: no array is indexed by a run-time value)
#pragma unroll
      for (int r = 0; r < B; ++r)
#pragma unroll
        for (int c = 0; c < B; ++c)
          if (t == r * B + c) v = c < r ? a[r][c] : (c == r ? 1.0 : 0.0);
      D.L[diag + t] = v;
    }
    if (t >= 64 && t < 64 + B) {
      double dv = 0.0, yv = 0.0;
#pragma unroll
      for (int r = 0; r < B; ++r)
        if (t - 64 == r) { dv = dd[r]; yv = yy[r]; }
      D.d[(size_t)j * B + t - 64] = dv;
      D.y[(size_t)j * B + t - 64] = yv;
    }
    // ---- the rows below: L_ij = S_ij L_jj^-T D_j^-1, and y_i -= L_ij y_j ----
    if (one) {
      if (t >= B && t < nItems) {
        double l[B];
        const double dot = envelope_below_line<B>(acc, a, dd, yy, l);
#pragma unroll
        for (int c = 0; c < B; ++c) mine[c] = l[c];
        D.y[(size_t)myRow * B + (t % B)] -= dot;
      }
    } else {
      for (int item = B + t; item < nItems; item += NT) {
        const int w = item / B, r = item - w * B;
        const int i = D.colRows[cs + w - 1];
        double* o = D.L + ((size_t)D.rowOff[i] + (j - D.rowFirst[i])) * BB + r * B;
        double s[B], l[B];
#pragma unroll
        for (int c = 0; c < B; ++c) s[c] = o[c];
        const double dot = envelope_below_line<B>(s, a, dd, yy, l);
#pragma unroll
        for (int c = 0; c < B; ++c) o[c] = l[c];
        D.y[(size_t)i * B + r] -= dot;
      }
    }
    __threadfence_block();
    __syncthreads();
  }
  return ok;
}

// x = L^-T D^-1 y behind a factorisation that succeeded: row i, once final, is taken out of the rows above it.  Called by every lane of one
// workgroup of NT; x is final for every lane when it returns.
template <int B, int NT>
__device__ __forceinline__ void envelope_backsub(const EnvelopeSys& D) {
  constexpr int BB = B * B;
  __shared__ double sx[B];
  const int t = threadIdx.x, n = D.n;
  for (int i = t; i < B * n; i += NT) D.x[i] = D.y[i] / D.d[i];
  __threadfence_block();
  __syncthreads();
  for (int i = n - 1; i >= 0; --i) {
    const int fi = D.rowFirst[i];
    const size_t rowI = (size_t)D.rowOff[i];
    if (t == 0) {   // x_i = L_ii^-T z_i
      const double* Ld = D.L + ((size_t)D.rowOff[i + 1] - 1) * BB;
      double z[B], xx[B];
#pragma unroll
      for (int r = 0; r < B; ++r) z[r] = D.x[(size_t)i * B + r];
#pragma unroll
      for (int r = B - 1; r >= 0; --r) {
        double v = z[r];
#pragma unroll
        for (int p = r + 1; p < B; ++p) v -= Ld[p * B + r] * xx[p];
        xx[r] = v;
      }
#pragma unroll
      for (int r = 0; r < B; ++r) { sx[r] = xx[r]; D.x[(size_t)i * B + r] = xx[r]; }
    }
    __syncthreads();
    const int cnt = (i - fi) * B;
    for (int item = t; item < cnt; item += NT) {
      const int kk = item / B, c = item - kk * B;
      const double* lik = D.L + (rowI + kk) * BB;
      double dot = 0;
#pragma unroll
      for (int r = 0; r < B; ++r) dot += lik[r * B + c] * sx[r];
      D.x[(size_t)(fi + kk) * B + c] -= dot;
    }
    __threadfence_block();
    __syncthreads();
  }
}

}  // namespace
