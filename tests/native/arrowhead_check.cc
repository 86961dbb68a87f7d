// The block steps of include/morb/arrowhead_math.h, run serially on random symmetric positive definite arrowheads and compared with a plain
// dense Cholesky written here.  Built by tests/test_inertial_optimization_cpu.py with -fsanitize=address,undefined; prints "arrowhead ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "morb/arrowhead_math.h"

namespace {

using morbarrow::NF;
using morbarrow::NG;

struct Arrow {
  int N;
  std::vector<double> T, O, F, C, rg;   // as solve_serial takes them
  std::vector<double> A, b;             // the same system, dense (lambda not included)
};

// A = M^T M over random "links" with the arrowhead's sparsity + a little on the diagonal: positive definite by construction.  zeroLink: the
// link whose off-diagonal block is zero (a broken chain), -1 for none.
Arrow make(int N, unsigned seed, int zeroLink) {
  std::mt19937_64 rng(seed);
  std::normal_distribution<double> nd(0.0, 1.0);
  const int m = 3 * N + NG;
  Arrow a;
  a.N = N;
  a.A.assign((size_t)m * m, 0.0);
  a.b.assign(m, 0.0);
  for (int k = 0; k < N; ++k) {
    // rows that touch velocity k - 1 (unless broken or k == 0), velocity k and the border
    const bool prev = k > 0 && k != zeroLink;
    for (int row = 0; row < 9; ++row) {
      std::vector<double> j(m, 0.0);
      if (prev) for (int c = 0; c < 3; ++c) j[3 * (k - 1) + c] = nd(rng);
      for (int c = 0; c < 3; ++c) j[3 * k + c] = nd(rng);
      for (int c = 0; c < NG; ++c) j[3 * N + c] = nd(rng);
      const double w = std::exp(0.5 * nd(rng));
      for (int r = 0; r < m; ++r) if (j[r] != 0.0) for (int c = 0; c < m; ++c) a.A[(size_t)r * m + c] += w * j[r] * j[c];
    }
  }
  for (int i = 0; i < m; ++i) { a.A[(size_t)i * m + i] += 1e-3; a.b[i] = nd(rng); }
  a.T.assign(9 * N, 0.0); a.O.assign(9 * N, 0.0); a.F.assign((size_t)3 * N * NF, 0.0); a.C.assign(NG * NG, 0.0); a.rg.assign(NG, 0.0);
  for (int k = 0; k < N; ++k)
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) {
        a.T[9 * k + r * 3 + c] = a.A[(size_t)(3 * k + r) * m + 3 * k + c];
        if (k > 0) a.O[9 * k + r * 3 + c] = a.A[(size_t)(3 * k + r) * m + 3 * (k - 1) + c];
      }
      for (int c = 0; c < NG; ++c) a.F[(size_t)(3 * k + r) * NF + c] = a.A[(size_t)(3 * k + r) * m + 3 * N + c];
      a.F[(size_t)(3 * k + r) * NF + NG] = a.b[3 * k + r];
    }
  for (int r = 0; r < NG; ++r) { for (int c = 0; c < NG; ++c) a.C[r * NG + c] = a.A[(size_t)(3 * N + r) * m + 3 * N + c]; a.rg[r] = a.b[3 * N + r]; }
  return a;
}

// dense Cholesky A = L L^T and the two substitutions; false when a pivot is not positive
bool cholesky_solve(int m, std::vector<double> A, const std::vector<double>& b, std::vector<double>& x) {
  for (int j = 0; j < m; ++j) {
    double d = A[(size_t)j * m + j];
    for (int k = 0; k < j; ++k) d -= A[(size_t)j * m + k] * A[(size_t)j * m + k];
    if (!(d > 0)) return false;
    d = std::sqrt(d);
    A[(size_t)j * m + j] = d;
    for (int r = j + 1; r < m; ++r) {
      double s = A[(size_t)r * m + j];
      for (int k = 0; k < j; ++k) s -= A[(size_t)r * m + k] * A[(size_t)j * m + k];
      A[(size_t)r * m + j] = s / d;
    }
  }
  x = b;
  for (int r = 0; r < m; ++r) { double s = x[r]; for (int c = 0; c < r; ++c) s -= A[(size_t)r * m + c] * x[c]; x[r] = s / A[(size_t)r * m + r]; }
  for (int r = m - 1; r >= 0; --r) { double s = x[r]; for (int c = r + 1; c < m; ++c) s -= A[(size_t)c * m + r] * x[c]; x[r] = s / A[(size_t)r * m + r]; }
  return true;
}

double check(const Arrow& a, double lambda, bool expectOk) {
  const int N = a.N, m = 3 * N + NG;
  std::vector<double> Dinv(9 * N), Fp((size_t)3 * N * NF), x(3 * N), g(NG);
  const bool ok = morbarrow::solve_serial(N, a.T.data(), a.O.data(), a.F.data(), a.C.data(), a.rg.data(), lambda, Dinv.data(), Fp.data(), x.data(), g.data());
  if (ok != expectOk) { std::printf("N %d lambda %g: solve_serial returned %d\n", N, lambda, (int)ok); std::exit(1); }
  if (!ok) return 0.0;
  std::vector<double> A = a.A, xs(m), xd;
  for (int i = 0; i < m; ++i) A[(size_t)i * m + i] += lambda;
  for (int i = 0; i < 3 * N; ++i) xs[i] = x[i];
  for (int i = 0; i < NG; ++i) xs[3 * N + i] = g[i];
  double rn = 0, bn = 0;
  for (int r = 0; r < m; ++r) { double s = -a.b[r]; for (int c = 0; c < m; ++c) s += A[(size_t)r * m + c] * xs[c]; rn += s * s; bn += a.b[r] * a.b[r]; }
  const double rel = std::sqrt(rn / bn);
  if (!cholesky_solve(m, A, a.b, xd)) { std::printf("dense Cholesky failed\n"); std::exit(1); }
  double dn = 0, xn = 0;
  for (int i = 0; i < m; ++i) { dn += (xs[i] - xd[i]) * (xs[i] - xd[i]); xn += xd[i] * xd[i]; }
  if (!(rel <= 1e-10)) { std::printf("N %d lambda %g: relative residual %.3e (solution differs from Cholesky's by %.3e)\n", N, lambda, rel, std::sqrt(dn / xn)); std::exit(1); }
  return rel;
}

}  // namespace

int main() {
  const int sizes[5] = {1, 2, 3, 17, 200};
  const double lambdas[5] = {0.0, 1e-5, 1.0, 1e3, 1e6};
  double worst = 0;
  unsigned seed = 1;
  for (int N : sizes)
    for (double lambda : lambdas) {
      worst = std::fmax(worst, check(make(N, seed++, -1), lambda, true));
      if (N >= 3) worst = std::fmax(worst, check(make(N, seed++, N / 2), lambda, true));   // a zero off-diagonal block in the middle
    }
  {  // not positive definite: a negative diagonal block in the middle of the chain, and one in the corner
    Arrow a = make(17, 99, -1);
    a.T[9 * 8 + 4] = -1.0; a.A[(size_t)(3 * 8 + 1) * (3 * 17 + NG) + 3 * 8 + 1] = -1.0;
    check(a, 0.0, false);
    Arrow c = make(3, 98, -1);
    c.C[4 * NG + 4] = -50.0;
    check(c, 1.0, false);
  }
  std::printf("arrowhead ok (worst relative residual %.2e)\n", worst);
  return 0;
}
