// CPU oracle of Optimizer::OptimizeEssentialGraph on the flattened graph (include/morb_hip.h: morb_optimize_essential_graph): an Eigen-free
// FP64 restatement of g2o's EdgeSim3 / VertexSim3Expmap (Sim3 log, exponential, product and inverse with g2o's eps branches), the numeric
// Jacobians of BaseBinaryEdge::linearizeOplus (central differences, delta = 1e-9), constructQuadraticForm's non-robust branch summed in edge
// order, g2o's Levenberg-Marquardt (setUserLambdaInit(1e-16), optimize(20)) and the point correction.  The linear system is solved by a plain
// scalar skyline LDL^T (row envelopes) — written independently of the library's block-column schedule.
// -DEG_ORACLE_REVERSE: the edges are visited in reverse wherever a sum runs over them (the second build of the tests).
// -DEG_ORACLE_NUDGE, -DEG_ORACLE_JITTER: a third build, for the corpus selection (below).
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct Sim3 { double q[4], t[3], s; };   // q = x y z w

// -DEG_ORACLE_NUDGE: acos and log inside Sim3::log land one ulp towards zero, as another libm's might (a third build, for judging how far the
// last bit of the two functions carries through the 1e-9 differences)
#ifdef EG_ORACLE_NUDGE
double acos_(double x) { return nextafter(acos(x), 0.0); }
double log_(double x) { return nextafter(log(x), 0.0); }
#else
double acos_(double x) { return acos(x); }
double log_(double x) { return log(x); }
#endif

void q_rotate(const double* q, const double* v, double* o) {   // QuaternionBase::_transformVector
  const double ux = q[0], uy = q[1], uz = q[2], w = q[3];
  double a = uy * v[2] - uz * v[1], b = uz * v[0] - ux * v[2], c = ux * v[1] - uy * v[0];
  a += a; b += b; c += c;
  o[0] = v[0] + w * a + (uy * c - uz * b);
  o[1] = v[1] + w * b + (uz * a - ux * c);
  o[2] = v[2] + w * c + (ux * b - uy * a);
}
Sim3 mul(const Sim3& a, const Sim3& b) {
  Sim3 r;
  const double *p = a.q, *o = b.q;
  r.q[3] = p[3] * o[3] - p[0] * o[0] - p[1] * o[1] - p[2] * o[2];
  r.q[0] = p[3] * o[0] + p[0] * o[3] + p[1] * o[2] - p[2] * o[1];
  r.q[1] = p[3] * o[1] + p[1] * o[3] + p[2] * o[0] - p[0] * o[2];
  r.q[2] = p[3] * o[2] + p[2] * o[3] + p[0] * o[1] - p[1] * o[0];
  double rt[3];
  q_rotate(a.q, b.t, rt);
  for (int i = 0; i < 3; ++i) r.t[i] = a.s * rt[i] + a.t[i];
  r.s = a.s * b.s;
  return r;
}
void map(const Sim3& S, const double* x, double* o) {
  double r[3];
  q_rotate(S.q, x, r);
  for (int i = 0; i < 3; ++i) o[i] = S.s * r[i] + S.t[i];
}
Sim3 inverse(const Sim3& S) {
  Sim3 r;
  r.q[0] = -S.q[0]; r.q[1] = -S.q[1]; r.q[2] = -S.q[2]; r.q[3] = S.q[3];
  const double ms = -1. / S.s;
  const double v[3] = {ms * S.t[0], ms * S.t[1], ms * S.t[2]};
  q_rotate(r.q, v, r.t);
  r.s = 1. / S.s;
  return r;
}
void R_to_q(const double* m, double* q) {   // Quaterniond(Matrix3d)
  double t = m[0] + m[4] + m[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t;
    q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
    q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
  }
}
Sim3 sim3_exp(const double* u) {   // Sim3(const Vector7d& update)
  const double w0 = u[0], w1 = u[1], w2 = u[2], sigma = u[6];
  const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
  const double Om[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
  double Om2[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Om2[i * 3 + j] = Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j] + Om[i * 3 + 2] * Om[6 + j];
  const double s = exp(sigma);
  const double eps = 0.00001;
  double A, B, C, R[9];
  const bool smallRot = theta < eps;
  if (fabs(sigma) < eps) {
    C = 1;
    if (smallRot) { A = 1. / 2.; B = 1. / 6.; }
    else {
      const double theta2 = theta * theta;
      A = (1 - cos(theta)) / (theta2);
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    C = (s - 1) / sigma;
    if (smallRot) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
    } else {
      const double a = s * sin(theta), b = s * cos(theta);
      const double theta2 = theta * theta, sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  if (smallRot) {
    for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + Om[i] + Om2[i];
  } else {
    const double f1 = sin(theta) / theta, f2 = (1 - cos(theta)) / (theta * theta);
    for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + f1 * Om[i] + f2 * Om2[i];
  }
  Sim3 r;
  R_to_q(R, r.q);
  double W[9];
  for (int i = 0; i < 9; ++i) W[i] = A * Om[i] + B * Om2[i] + C * ((i % 4 == 0) ? 1.0 : 0.0);
  for (int i = 0; i < 3; ++i) r.t[i] = W[i * 3] * u[3] + W[i * 3 + 1] * u[4] + W[i * 3 + 2] * u[5];
  r.s = s;
  return r;
}
// Sim3::log (types/sim3.h:148-230); *branch: bit 0 |sigma| < eps, bit 1 d > 1 - eps
void sim3_log(const Sim3& S, double* res, int* branch = nullptr) {
  const double sigma = log_(S.s);
  const double x = S.q[0], y = S.q[1], z = S.q[2], w = S.q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  const double R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double eps = 0.00001;
  double A, B, C, om[3];
  if (branch) *branch = (fabs(sigma) < eps ? 1 : 0) | (d > 1 - eps ? 2 : 0);
  if (fabs(sigma) < eps) {
    C = 1;
    if (d > 1 - eps) {
      for (int i = 0; i < 3; ++i) om[i] = 0.5 * dR[i];
      A = 1. / 2.; B = 1. / 6.;
    } else {
      const double theta = acos_(d);
      const double theta2 = theta * theta;
      const double f = theta / (2 * sqrt(1 - d * d));
      for (int i = 0; i < 3; ++i) om[i] = f * dR[i];
      A = (1 - cos(theta)) / (theta2);
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    C = (S.s - 1) / sigma;
    if (d > 1 - eps) {
      const double sigma2 = sigma * sigma;
      for (int i = 0; i < 3; ++i) om[i] = 0.5 * dR[i];
      A = ((sigma - 1) * S.s + 1) / (sigma2);
      B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
    } else {
      const double theta = acos_(d);
      const double f = theta / (2 * sqrt(1 - d * d));
      for (int i = 0; i < 3; ++i) om[i] = f * dR[i];
      const double theta2 = theta * theta;
      const double a = S.s * sin(theta);
      const double b = S.s * cos(theta);
      const double c = theta2 + sigma * sigma;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  const double Om[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
  double a[3][4];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      const double o2 = Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j] + Om[i * 3 + 2] * Om[6 + j];
      a[i][j] = A * Om[i * 3 + j] + B * o2 + C * (i == j ? 1.0 : 0.0);
    }
    a[i][3] = S.t[i];
  }
  // W.lu().solve(t): PartialPivLU
  for (int k = 0; k < 3; ++k) {
    int p = k;
    double big = fabs(a[k][k]);
    for (int i = k + 1; i < 3; ++i) if (fabs(a[i][k]) > big) { big = fabs(a[i][k]); p = i; }
    if (p != k) for (int j = 0; j < 4; ++j) { const double v = a[k][j]; a[k][j] = a[p][j]; a[p][j] = v; }
    for (int i = k + 1; i < 3; ++i) {
      a[i][k] /= a[k][k];
      for (int j = k + 1; j < 3; ++j) a[i][j] -= a[i][k] * a[k][j];
    }
  }
  const double y0 = a[0][3], y1 = a[1][3] - a[1][0] * y0, y2 = a[2][3] - (a[2][0] * y0 + a[2][1] * y1);
  const double u2 = y2 / a[2][2];
  const double u1 = (y1 - a[1][2] * u2) / a[1][1];
  const double u0 = (y0 - (a[0][1] * u1 + a[0][2] * u2)) / a[0][0];
  res[0] = om[0]; res[1] = om[1]; res[2] = om[2];
  res[3] = u0; res[4] = u1; res[5] = u2;
  res[6] = sigma;
}

Sim3 load(const double* p) { Sim3 s; memcpy(&s, p, sizeof s); return s; }
void store(double* p, const Sim3& s) { memcpy(p, &s, sizeof s); }

void edge_error(const Sim3& M, const Sim3& Si, const Sim3& Sj, double* e) { sim3_log(mul(mul(M, Si), inverse(Sj)), e); }
Sim3 oplus(const Sim3& S, const double* update, bool fixScale) {   // VertexSim3Expmap::oplusImpl
  double u[7];
  for (int i = 0; i < 7; ++i) u[i] = update[i];
  if (fixScale) u[6] = 0;
  return mul(sim3_exp(u), S);
}

struct Graph {
  int nKF, nE, n;
  const uint8_t* flags;
  const int *eI, *eJ;
  const double* eS;
  std::vector<Sim3> S;
  std::vector<int> col;          // vertex -> block row, or -1
  std::vector<int> first;        // scalar row -> first scalar column of its envelope
  std::vector<std::vector<double>> H;   // scalar rows over their envelopes
  std::vector<double> b;
  std::vector<double> J;         // [nE][2][49]
  std::vector<double> err;       // [nE][7]
};

template <class F>
void for_edges(int nE, F&& f) {
#ifdef EG_ORACLE_REVERSE
  for (int e = nE - 1; e >= 0; --e) f(e);
#else
  for (int e = 0; e < nE; ++e) f(e);
#endif
}

double active_chi2(const Graph& g, const std::vector<Sim3>& X) {
  double chi = 0;
  for_edges(g.nE, [&](int e) {
    double er[7];
    edge_error(load(g.eS + (size_t)e * 8), X[g.eI[e]], X[g.eJ[e]], er);
    double c = 0;
    for (int k = 0; k < 7; ++k) c += er[k] * er[k];
    chi += c;
  });
  return chi;
}

void linearize(Graph& g) {
  const double delta = 1e-9, scalar = 1.0 / (2 * delta);
  for (int e = 0; e < g.nE; ++e) {
    const Sim3 M = load(g.eS + (size_t)e * 8), Si = g.S[g.eI[e]], Sj = g.S[g.eJ[e]];
    edge_error(M, Si, Sj, &g.err[(size_t)e * 7]);
    for (int side = 0; side < 2; ++side) {
      const int v = side ? g.eJ[e] : g.eI[e];
      if (g.flags[v] & 1) continue;
      double* J = &g.J[((size_t)e * 2 + side) * 49];
      for (int d = 0; d < 7; ++d) {
        double add[7] = {0, 0, 0, 0, 0, 0, 0}, ep[7], em[7];
        add[d] = delta;
        const Sim3 Sp = oplus(side ? Sj : Si, add, (g.flags[v] & 2) != 0);
        add[d] = -delta;
        const Sim3 Sm = oplus(side ? Sj : Si, add, (g.flags[v] & 2) != 0);
        if (side) { edge_error(M, Si, Sp, ep); edge_error(M, Si, Sm, em); }
        else { edge_error(M, Sp, Sj, ep); edge_error(M, Sm, Sj, em); }
        for (int r = 0; r < 7; ++r) J[r * 7 + d] = scalar * (ep[r] - em[r]);
      }
    }
  }
}

// constructQuadraticForm of every edge: lower triangle of H in the row envelopes, b
void build(Graph& g) {
  for (auto& row : g.H) std::fill(row.begin(), row.end(), 0.0);
  std::fill(g.b.begin(), g.b.end(), 0.0);
  auto at = [&](int r, int c) -> double& { return g.H[r][c - g.first[r]]; };
  for_edges(g.nE, [&](int e) {
    const int a = g.col[g.eI[e]], bcol = g.col[g.eJ[e]];
    const double *Ji = &g.J[((size_t)e * 2) * 49], *Jj = &g.J[((size_t)e * 2 + 1) * 49], *er = &g.err[(size_t)e * 7];
    for (int side = 0; side < 2; ++side) {
      const int blk = side ? bcol : a;
      if (blk < 0) continue;
      const double* Jx = side ? Jj : Ji;
      for (int r = 0; r < 7; ++r) {
        double v = 0;
        for (int k = 0; k < 7; ++k) v += Jx[k * 7 + r] * (-er[k]);
        g.b[blk * 7 + r] += v;
        for (int c = 0; c <= r; ++c) {
          double h = 0;
          for (int k = 0; k < 7; ++k) h += Jx[k * 7 + r] * Jx[k * 7 + c];
          at(blk * 7 + r, blk * 7 + c) += h;
        }
      }
    }
    if (a >= 0 && bcol >= 0) {
      const double *Jr = a > bcol ? Ji : Jj, *Jc = a > bcol ? Jj : Ji;
      const int br = a > bcol ? a : bcol, bc = a > bcol ? bcol : a;
      for (int r = 0; r < 7; ++r)
        for (int c = 0; c < 7; ++c) {
          double h = 0;
          for (int k = 0; k < 7; ++k) h += Jr[k * 7 + r] * Jc[k * 7 + c];
          at(br * 7 + r, bc * 7 + c) += h;
        }
    }
  });
}

// (H + lambda I) x = b by a scalar skyline LDL^T; false: a pivot is not positive
bool solve(const Graph& g, double lambda, std::vector<double>& x) {
  const int N = 7 * g.n;
  std::vector<std::vector<double>> L(g.H);
  std::vector<double> d(N);
  for (int i = 0; i < N; ++i) {
    const int fi = g.first[i];
    L[i][i - fi] += lambda;
#ifdef EG_ORACLE_JITTER   // (= 0, 1, ...: the pattern) every entry off by up to three ulp: what another elimination schedule's rounding does to the matrix
    for (int j = fi; j <= i; ++j) L[i][j - fi] *= (1 + 2.2e-16 * (((i * 31 + j * 17 + EG_ORACLE_JITTER) % 7) - 3));
#endif
    for (int j = fi; j <= i; ++j) {
      const int fj = g.first[j];
      double s = L[i][j - fi];
      for (int k = fi > fj ? fi : fj; k < j; ++k) s -= (L[i][k - fi] * d[k]) * L[j][k - fj];
      if (j < i) L[i][j - fi] = s / d[j];
      else { d[i] = s; if (!(s > 0)) return false; }
    }
  }
  std::vector<double> y(g.b);
  for (int i = 0; i < N; ++i) { const int fi = g.first[i]; for (int k = fi; k < i; ++k) y[i] -= L[i][k - fi] * y[k]; }
  for (int i = 0; i < N; ++i) y[i] /= d[i];
  for (int i = N - 1; i >= 0; --i) { const int fi = g.first[i]; for (int k = fi; k < i; ++k) y[k] -= L[i][k - fi] * y[i]; }
  x = y;
  return true;
}

void setup(Graph& g, int nKF, const double* S, const uint8_t* flags, int nE, const int* eI, const int* eJ, const double* eS) {
  g.nKF = nKF; g.nE = nE; g.flags = flags; g.eI = eI; g.eJ = eJ; g.eS = eS;
  g.S.resize(nKF);
  for (int v = 0; v < nKF; ++v) g.S[v] = load(S + (size_t)v * 8);
  std::vector<char> used(nKF, 0);
  for (int e = 0; e < nE; ++e) used[eI[e]] = used[eJ[e]] = 1;
  g.col.assign(nKF, -1);
  g.n = 0;
  for (int v = 0; v < nKF; ++v) if (!(flags[v] & 1) && used[v]) g.col[v] = g.n++;
  std::vector<int> bf(g.n);
  for (int r = 0; r < g.n; ++r) bf[r] = r;
  for (int e = 0; e < nE; ++e) {
    const int a = g.col[eI[e]], b = g.col[eJ[e]];
    if (a >= 0 && b >= 0) { const int hi = a > b ? a : b, lo = a > b ? b : a; if (lo < bf[hi]) bf[hi] = lo; }
  }
  g.first.resize(7 * g.n); g.H.resize(7 * g.n); g.b.assign(7 * g.n, 0.0);
  for (int i = 0; i < 7 * g.n; ++i) { g.first[i] = 7 * bf[i / 7]; g.H[i].assign(i - g.first[i] + 1, 0.0); }
  g.J.assign((size_t)nE * 98, 0.0); g.err.assign((size_t)nE * 7, 0.0);
}

}  // namespace

extern "C" {

void eg_oracle_exp(const double* u7, double* out8) { store(out8, sim3_exp(u7)); }
int eg_oracle_log(const double* S8, double* out7) { int br = 0; sim3_log(load(S8), out7, &br); return br; }
void eg_oracle_mul(const double* a8, const double* b8, double* out8) { store(out8, mul(load(a8), load(b8))); }
void eg_oracle_inverse(const double* a8, double* out8) { store(out8, inverse(load(a8))); }
// bit 0: some edge's error at the entry estimates takes the |sigma| < eps branch; bit 1: some takes d > 1 - eps; bit 2: some takes neither of the two
int eg_oracle_branches(int nKF, const double* S, int nE, const int* eI, const int* eJ, const double* eS) {
  int seen = 0;
  for (int e = 0; e < nE; ++e) {
    double er[7];
    int br = 0;
    sim3_log(mul(mul(load(eS + (size_t)e * 8), load(S + (size_t)eI[e] * 8)), inverse(load(S + (size_t)eJ[e] * 8))), er, &br);
    seen |= (br & 1) | (br & 2) | (br == 0 ? 4 : 0);
  }
  (void)nKF;
  return seen;
}

// the quadratic form at the entry estimates as a dense symmetric matrix Hd [7n][7n] and bd [7n]; returns n
int eg_oracle_system(int nKF, const double* S, const uint8_t* flags, int nE, const int* eI, const int* eJ, const double* eS, double* Hd, double* bd) {
  Graph g;
  setup(g, nKF, S, flags, nE, eI, eJ, eS);
  linearize(g);
  build(g);
  const int N = 7 * g.n;
  if (Hd) {
    for (int i = 0; i < N * N; ++i) Hd[i] = 0;
    for (int i = 0; i < N; ++i)
      for (int j = g.first[i]; j <= i; ++j) Hd[i * N + j] = Hd[j * N + i] = g.H[i][j - g.first[i]];
    for (int i = 0; i < N; ++i) bd[i] = g.b[i];
  }
  return g.n;
}

// the whole call: S in place, the points in place, stats4 = {outer iterations, trials, vertices in the system, envelope blocks}, chi2[2]
void eg_oracle_run(int nKF, double* S, const uint8_t* flags, int nE, const int* eI, const int* eJ, const double* eS, int nMP, float* mp,
                   const int* mpRef, int* stats4, double* chi2) {
  Graph g;
  setup(g, nKF, S, flags, nE, eI, eJ, eS);
  for (int k = 0; k < 4; ++k) stats4[k] = 0;
  chi2[0] = chi2[1] = 0;
  if (!g.n) return;
  const std::vector<Sim3> S0 = g.S;
  int blocks = 0;
  for (int r = 0; r < g.n; ++r) blocks += r - g.first[7 * r] / 7 + 1;
  stats4[2] = g.n; stats4[3] = blocks;
  // OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:61-169) under SparseOptimizer::optimize(20)
  std::vector<double> x(7 * g.n, 0.0);
  double lambda = 0, ni = 2, currentChi = active_chi2(g, g.S);
  chi2[0] = currentChi;
  int nBad = 0, its = 0, trials = 0;
  for (int it = 0; it < 20; ++it) {
    linearize(g);
    build(g);
    const double iniChi = currentChi;
    if (it == 0) { lambda = 1e-16; ni = 2; nBad = 0; }   // setUserLambdaInit(1e-16)
    double rho = 0;
    int qmax = 0;
    do {
      const bool ok2 = solve(g, lambda, x);
      std::vector<Sim3> T(g.S);
      for (int v = 0; v < nKF; ++v) if (g.col[v] >= 0) T[v] = oplus(g.S[v], &x[g.col[v] * 7], (flags[v] & 2) != 0);
      double tempChi = active_chi2(g, T);
      if (!ok2) tempChi = DBL_MAX;
      rho = (currentChi - tempChi);
      double scale = 0;
      for (int j = 0; j < 7 * g.n; ++j) scale += x[j] * (lambda * x[j] + g.b[j]);
      scale += 1e-3;
      rho /= scale;
      if (rho > 0 && std::isfinite(tempChi)) {
        double alpha = 1. - pow(2 * rho - 1, 3);
        alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
        const double scaleFactor = 1. / 3. > alpha ? 1. / 3. : alpha;
        lambda *= scaleFactor;
        ni = 2;
        currentChi = tempChi;
        g.S = T;
      } else {
        lambda *= ni;
        ni *= 2;
      }
      ++qmax; ++trials;
    } while (rho < 0 && qmax < 10);
    ++its;
    if (qmax == 10 || rho == 0 || !(rho == rho)) break;
    if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
    if (nBad >= 3) break;
  }
  stats4[0] = its; stats4[1] = trials;
  chi2[1] = currentChi;
  for (int v = 0; v < nKF; ++v) store(S + (size_t)v * 8, g.S[v]);
  for (int m = 0; m < nMP; ++m) {
    const int v = mpRef[m];
    if (v < 0) continue;
    const Sim3 Swr = inverse(g.S[v]);
    const double P[3] = {(double)mp[m * 3], (double)mp[m * 3 + 1], (double)mp[m * 3 + 2]};
    double a[3], o[3];
    map(S0[v], P, a);
    map(Swr, a, o);
    for (int k = 0; k < 3; ++k) mp[m * 3 + k] = (float)o[k];
  }
}

}
