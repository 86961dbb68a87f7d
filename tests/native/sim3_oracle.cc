// CPU oracle of Optimizer::OptimizeSim3 (reference src/Optimizer.cc:2065-2322): an independent FP64 restatement, one problem per
// call, built by tests/test_sim3_cpu.py with g++ -O2 -ffp-contract=off and loaded with ctypes.
//   g2o: OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:61-169), SparseOptimizer::optimize,
//        BaseBinaryEdge::linearizeOplus (numeric, delta 1e-9) + constructQuadraticForm, RobustKernelHuber, VertexSim3Expmap::oplusImpl,
//        g2o::Sim3 (types/sim3.h), LinearSolverDense = Eigen::LDLT (pivoted);
//   cameras: Pinhole::project(Vector3d), KannalaBrandt8::project(Vector3d) with its float atan2f / sqrtf.
// Everything calls the host libm (exp, sin, cos, pow, atan2f), as the reference does.  Sums run in g2o's edge order.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct Sim3 { double q[4]; double t[3]; double s; };   // q = x y z w
struct Cam { bool kb8; float p[8]; };

void rotate(const double* q, const double* v, double* out) {   // Eigen's _transformVector: v + w uv + q.vec() x uv, uv = 2 q.vec() x v
  double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
  for (double& u : uv) u += u;
  const double cx = q[1] * uv[2] - q[2] * uv[1], cy = q[2] * uv[0] - q[0] * uv[2], cz = q[0] * uv[1] - q[1] * uv[0];
  out[0] = v[0] + q[3] * uv[0] + cx;
  out[1] = v[1] + q[3] * uv[1] + cy;
  out[2] = v[2] + q[3] * uv[2] + cz;
}

Sim3 mul(const Sim3& a, const Sim3& b) {
  Sim3 r;
  const double* p = a.q; const double* o = b.q;
  r.q[3] = p[3] * o[3] - p[0] * o[0] - p[1] * o[1] - p[2] * o[2];
  r.q[0] = p[3] * o[0] + p[0] * o[3] + p[1] * o[2] - p[2] * o[1];
  r.q[1] = p[3] * o[1] + p[1] * o[3] + p[2] * o[0] - p[0] * o[2];
  r.q[2] = p[3] * o[2] + p[2] * o[3] + p[0] * o[1] - p[1] * o[0];
  double v[3];
  rotate(a.q, b.t, v);
  for (int i = 0; i < 3; ++i) r.t[i] = a.s * v[i] + a.t[i];
  r.s = a.s * b.s;
  return r;
}

void map(const Sim3& S, const double* x, double* o) {
  double v[3];
  rotate(S.q, x, v);
  for (int i = 0; i < 3; ++i) o[i] = S.s * v[i] + S.t[i];
}

Sim3 inverse(const Sim3& S) {
  Sim3 r;
  r.q[0] = -S.q[0]; r.q[1] = -S.q[1]; r.q[2] = -S.q[2]; r.q[3] = S.q[3];
  const double f = -1. / S.s;
  double v[3];
  for (int i = 0; i < 3; ++i) v[i] = f * S.t[i];
  rotate(r.q, v, r.t);
  r.s = 1. / S.s;
  return r;
}

void quat_from_matrix(const double (&m)[3][3], double* q) {   // Eigen: largest of trace / diagonal
  double t = m[0][0] + m[1][1] + m[2][2];
  if (t > 0) {
    t = std::sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[2][1] - m[1][2]) * t;
    q[1] = (m[0][2] - m[2][0]) * t;
    q[2] = (m[1][0] - m[0][1]) * t;
    return;
  }
  int i = 0;
  if (m[1][1] > m[0][0]) i = 1;
  if (m[2][2] > m[i][i]) i = 2;
  int j = (i + 1) % 3, k = (j + 1) % 3;
  t = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
  q[i] = 0.5 * t;
  t = 0.5 / t;
  q[3] = (m[k][j] - m[j][k]) * t;
  q[j] = (m[j][i] + m[i][j]) * t;
  q[k] = (m[k][i] + m[i][k]) * t;
}

Sim3 expmap(const double* upd) {   // g2o::Sim3(const Vector7d&)
  const double sigma = upd[6];
  const double theta = std::sqrt(upd[0] * upd[0] + upd[1] * upd[1] + upd[2] * upd[2]);
  const double O[3][3] = {{0, -upd[2], upd[1]}, {upd[2], 0, -upd[0]}, {-upd[1], upd[0], 0}};
  double O2[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) O2[i][j] = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
  const double s = std::exp(sigma);
  const double eps = 0.00001;
  double A, B, C, R[3][3];
  auto rodrigues = [&]() {
    const double a = std::sin(theta) / theta, b = (1 - std::cos(theta)) / (theta * theta);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) R[i][j] = (i == j ? 1.0 : 0.0) + a * O[i][j] + b * O2[i][j];
  };
  auto small = [&]() {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) R[i][j] = (i == j ? 1.0 : 0.0) + O[i][j] + O2[i][j];
  };
  if (std::fabs(sigma) < eps) {
    C = 1;
    if (theta < eps) {
      A = 1. / 2.;
      B = 1. / 6.;
      small();
    } else {
      const double theta2 = theta * theta;
      A = (1 - std::cos(theta)) / (theta2);
      B = (theta - std::sin(theta)) / (theta2 * theta);
      rodrigues();
    }
  } else {
    C = (s - 1) / sigma;
    if (theta < eps) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
      small();
    } else {
      rodrigues();
      const double a = s * std::sin(theta), b = s * std::cos(theta);
      const double theta2 = theta * theta, sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  Sim3 r;
  quat_from_matrix(R, r.q);
  for (int i = 0; i < 3; ++i) {
    double W[3];
    for (int j = 0; j < 3; ++j) W[j] = A * O[i][j] + B * O2[i][j] + C * (i == j ? 1.0 : 0.0);
    r.t[i] = W[0] * upd[3] + W[1] * upd[4] + W[2] * upd[5];
  }
  r.s = s;
  return r;
}

void project(const Cam& c, const double* v, double* uv) {
  if (!c.kb8) {
    uv[0] = c.p[0] * v[0] / v[2] + c.p[2];
    uv[1] = c.p[1] * v[1] / v[2] + c.p[3];
    return;
  }
  const double x2_plus_y2 = v[0] * v[0] + v[1] * v[1];
  const double theta = atan2f(sqrtf(x2_plus_y2), v[2]);
  const double psi = atan2f(v[1], v[0]);
  const double theta2 = theta * theta;
  const double theta3 = theta * theta2;
  const double theta5 = theta3 * theta2;
  const double theta7 = theta5 * theta2;
  const double theta9 = theta7 * theta2;
  const double r = theta + c.p[4] * theta3 + c.p[5] * theta5 + c.p[6] * theta7 + c.p[7] * theta9;
  uv[0] = c.p[0] * r * std::cos(psi) + c.p[2];
  uv[1] = c.p[1] * r * std::sin(psi) + c.p[3];
}

struct Edge {            // one of EdgeSim3ProjectXYZ (inverse = false) / EdgeInverseSim3ProjectXYZ (inverse = true)
  bool inverse;
  double X[3];           // the fixed point vertex
  double obs[2];
  double info;
  bool robust = true;
  double err[2] = {0, 0};
  double J[2][7];
};

struct Problem {
  Sim3 est;
  bool fixScale;
  Cam c1, c2;
  double delta;          // Huber delta
  std::vector<Edge> edges;
  std::vector<char> active;

  void computeError(Edge& e, const Sim3& S) const {
    double x[3], uv[2];
    if (!e.inverse) { map(S, e.X, x); project(c1, x, uv); }
    else { map(inverse(S), e.X, x); project(c2, x, uv); }
    e.err[0] = e.obs[0] - uv[0];
    e.err[1] = e.obs[1] - uv[1];
  }
  static double chi2(const Edge& e) { return e.err[0] * (e.info * e.err[0]) + e.err[1] * (e.info * e.err[1]); }
  double robustChi(const Edge& e, double* w) const {
    const double c = chi2(e);
    *w = 1.;
    if (!e.robust) return c;
    const double dsqr = delta * delta;
    if (c <= dsqr) return c;
    const double sq = std::sqrt(c);
    *w = delta / sq;
    return 2 * sq * delta - dsqr;
  }
  Sim3 oplus(const Sim3& S, const double* x) const {
    double u[7];
    std::memcpy(u, x, sizeof u);
    if (fixScale) u[6] = 0;
    return mul(expmap(u), S);
  }
  void computeActiveErrors(const Sim3& S) {
    for (size_t k = 0; k < edges.size(); ++k)
      if (active[k]) computeError(edges[k], S);
  }
  double activeRobustChi2() const {
    double chi = 0, w;
    for (size_t k = 0; k < edges.size(); ++k)
      if (active[k]) chi += robustChi(edges[k], &w);
    return chi;
  }
  void linearize(Edge& e) {
    const double dlt = 1e-9, scalar = 1.0 / (2 * dlt);
    const double bak[2] = {e.err[0], e.err[1]};
    double add[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int d = 0; d < 7; ++d) {
      add[d] = dlt;
      computeError(e, oplus(est, add));
      double eb[2] = {e.err[0], e.err[1]};
      add[d] = -dlt;
      computeError(e, oplus(est, add));
      eb[0] -= e.err[0];
      eb[1] -= e.err[1];
      add[d] = 0.0;
      e.J[0][d] = scalar * eb[0];
      e.J[1][d] = scalar * eb[1];
    }
    e.err[0] = bak[0];
    e.err[1] = bak[1];
  }
  // H (full, lower triangle filled) and b of the active edges, in edge order
  void buildSystem(double (&H)[7][7], double (&b)[7]) {
    std::memset(H, 0, sizeof H);
    std::memset(b, 0, sizeof b);
    for (size_t k = 0; k < edges.size(); ++k) {
      if (!active[k]) continue;
      Edge& e = edges[k];
      linearize(e);
      double w;
      robustChi(e, &w);
      const double wo = w * e.info;
      double omr[2] = {-(e.info * e.err[0]), -(e.info * e.err[1])};
      if (e.robust) { omr[0] *= w; omr[1] *= w; }
      for (int r = 0; r < 7; ++r) {
        b[r] += e.J[0][r] * omr[0] + e.J[1][r] * omr[1];
        for (int c = 0; c <= r; ++c) H[r][c] += (e.J[0][r] * wo) * e.J[0][c] + (e.J[1][r] * wo) * e.J[1][c];
      }
    }
  }
};

// Eigen::LDLT<MatrixXd>::compute + solve (lower triangle, diagonal pivoting); returns isPositive()
bool ldlt(double (&m)[7][7], const double* rhs, double* x) {
  const int n = 7;
  int tr[7];
  double tmp[7];
  int sign = 0;   // ZeroSign, PositiveSemiDef, NegativeSemiDef, Indefinite
  for (int k = 0; k < n; ++k) {
    int big = k;
    for (int i = k + 1; i < n; ++i)
      if (std::fabs(m[i][i]) > std::fabs(m[big][big])) big = i;
    tr[k] = big;
    if (big != k) {
      for (int j = 0; j < k; ++j) std::swap(m[k][j], m[big][j]);
      for (int i = big + 1; i < n; ++i) std::swap(m[i][k], m[i][big]);
      std::swap(m[k][k], m[big][big]);
      for (int i = k + 1; i < big; ++i) std::swap(m[i][k], m[big][i]);
    }
    if (k > 0) {
      for (int j = 0; j < k; ++j) tmp[j] = m[j][j] * m[k][j];
      double d = 0;
      for (int j = 0; j < k; ++j) d += m[k][j] * tmp[j];
      m[k][k] -= d;
      for (int i = k + 1; i < n; ++i)
        for (int j = 0; j < k; ++j) m[i][k] -= m[i][j] * tmp[j];
    }
    const double akk = m[k][k];
    const bool valid = std::fabs(akk) > 0;
    if (k == 0 && !valid) {
      sign = 0;
      for (int j = 0; j < n; ++j) tr[j] = j;
      break;
    }
    if (valid)
      for (int i = k + 1; i < n; ++i) m[i][k] /= akk;
    if (sign == 1) { if (akk < 0) sign = 3; }
    else if (sign == 2) { if (akk > 0) sign = 3; }
    else if (sign == 0) { if (akk > 0) sign = 1; else if (akk < 0) sign = 2; }
  }
  if (sign != 0 && sign != 1) return false;
  double y[7];
  std::memcpy(y, rhs, sizeof y);
  for (int k = 0; k < n; ++k) std::swap(y[k], y[tr[k]]);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < i; ++j) y[i] -= m[i][j] * y[j];
  for (int i = 0; i < n; ++i) y[i] = std::fabs(m[i][i]) > DBL_MIN ? y[i] / m[i][i] : 0.0;
  for (int i = n - 1; i >= 0; --i)
    for (int j = i + 1; j < n; ++j) y[i] -= m[j][i] * y[j];
  for (int k = n - 1; k >= 0; --k) std::swap(y[k], y[tr[k]]);
  std::memcpy(x, y, sizeof y);
  return true;
}

// optimizer.initializeOptimization(); optimizer.optimize(iterations); returns (iterations run, LM trials)
void optimize(Problem& P, int iterations, int* itOut, int* trOut) {
  double lambda = 0, x[7] = {0, 0, 0, 0, 0, 0, 0};
  int ni = 2, nBad = 0, its = 0, trials = 0;
  for (int it = 0; it < iterations; ++it) {
    P.computeActiveErrors(P.est);
    double currentChi = P.activeRobustChi2();
    const double iniChi = currentChi;
    double H[7][7], b[7];
    P.buildSystem(H, b);
    if (it == 0) {
      double maxDiagonal = 0.;
      for (int j = 0; j < 7; ++j) maxDiagonal = std::max(std::fabs(H[j][j]), maxDiagonal);
      lambda = 1e-5 * maxDiagonal;
      ni = 2;
      nBad = 0;
    }
    double rho = 0;
    int qmax = 0;
    do {
      double A[7][7];
      for (int r = 0; r < 7; ++r)
        for (int c = 0; c <= r; ++c) A[r][c] = A[c][r] = H[r][c];
      for (int j = 0; j < 7; ++j) A[j][j] += lambda;
      double xs[7];
      const bool ok2 = ldlt(A, b, xs);
      if (ok2) std::memcpy(x, xs, sizeof x);
      const Sim3 trial = P.oplus(P.est, x);
      P.computeActiveErrors(trial);
      double tempChi = P.activeRobustChi2();
      if (!ok2) tempChi = DBL_MAX;
      rho = currentChi - tempChi;
      double scale = 0.;
      for (int j = 0; j < 7; ++j) scale += x[j] * (lambda * x[j] + b[j]);
      scale += 1e-3;
      rho /= scale;
      if (rho > 0 && std::isfinite(tempChi)) {
        double alpha = 1. - std::pow((2 * rho - 1), 3);
        alpha = std::min(alpha, 2. / 3.);
        const double scaleFactor = std::max(1. / 3., alpha);
        lambda *= scaleFactor;
        ni = 2;
        currentChi = tempChi;
        P.est = trial;
      } else {
        lambda *= ni;
        ni *= 2;
      }
      qmax++;
      trials++;
    } while (rho < 0 && qmax < 10);
    its++;
    if (qmax == 10 || rho == 0) break;
    if ((iniChi - currentChi) * 1e3 < iniChi) nBad++;
    else nBad = 0;
    if (nBad >= 3) break;
  }
  *itOut = its;
  *trOut = trials;
}

}  // namespace

extern "C" {

// One problem.  Per KF1 feature i < n: entry bit 0 = vpMatches1[i] != NULL, bit 1 = pMP1 present, bit 2 = pMP1->isBad(), bit 3 =
// pMP2->isBad(); Xw1 / Xw2 world positions; i2 = pMP2's index in KF2; obs1 / inv1 = KF1 keypoint and mvInvLevelSigma2 of its
// octave; obs2 / inv2 = KF2 keypoint i2 (unused when i2 < 0) and the sigma of its octave (of mnTrackScaleLevel when i2 < 0).
// T1w / T2w: R row-major + t (float); cam: kind (0 pinhole, 1 KB8) + 8 parameters.  S12 in / out (qx qy qz qw tx ty tz s, written only
// when the function reaches its end); keep[i] = vpMatches1[i] != NULL on return; stats as morb_optimize_sim3_batch's.  Returns nIn.
int sim3_oracle_solve(int n, const uint8_t* entry, const float* Xw1, const float* Xw2, const int* i2v, const float* obs1, const float* inv1,
                      const float* obs2, const float* inv2, const float* T1w, const float* T2w, const float* cam1, const float* cam2, float th2,
                      int bFixScale, int bAllPoints, double* S12, uint8_t* keep, int* stats) {
  Problem P;
  P.fixScale = bFixScale != 0;
  P.c1.kb8 = cam1[0] != 0.f;
  P.c2.kb8 = cam2[0] != 0.f;
  for (int k = 0; k < 8; ++k) { P.c1.p[k] = cam1[1 + k]; P.c2.p[k] = cam2[1 + k]; }
  const float deltaHuber = std::sqrt(th2);
  P.delta = deltaHuber;
  for (int k = 0; k < 4; ++k) P.est.q[k] = S12[k];
  for (int k = 0; k < 3; ++k) P.est.t[k] = S12[4 + k];
  P.est.s = S12[7];
  std::vector<int> featOf;
  for (int i = 0; i < n; ++i) keep[i] = entry[i] & 1;
  for (int i = 0; i < n; ++i) {
    const uint8_t e = entry[i];
    if (!(e & 1)) continue;
    if (!(e & 2)) continue;             // nMatchWithoutMP
    if ((e & 4) || (e & 8)) continue;   // nBadMPs
    float P1[3], P2[3];
    for (int r = 0; r < 3; ++r) {
      P1[r] = T1w[r * 3] * Xw1[i * 3] + T1w[r * 3 + 1] * Xw1[i * 3 + 1] + T1w[r * 3 + 2] * Xw1[i * 3 + 2] + T1w[9 + r];
      P2[r] = T2w[r * 3] * Xw2[i * 3] + T2w[r * 3 + 1] * Xw2[i * 3 + 1] + T2w[r * 3 + 2] * Xw2[i * 3 + 2] + T2w[9 + r];
    }
    const int i2 = i2v[i];
    if (i2 < 0 && !bAllPoints) continue;
    if (P2[2] < 0) continue;
    Edge e12, e21;
    e12.inverse = false;
    for (int r = 0; r < 3; ++r) e12.X[r] = P2[r];
    e12.obs[0] = obs1[i * 2];
    e12.obs[1] = obs1[i * 2 + 1];
    e12.info = inv1[i];
    e21.inverse = true;
    for (int r = 0; r < 3; ++r) e21.X[r] = P1[r];
    if (i2 >= 0) {
      e21.obs[0] = obs2[i * 2];
      e21.obs[1] = obs2[i * 2 + 1];
    } else {
      float invz = 1 / P2[2];
      float x = P2[0] * invz;
      float y = P2[1] * invz;
      e21.obs[0] = x;
      e21.obs[1] = y;
    }
    e21.info = inv2[i];
    P.edges.push_back(e12);
    P.edges.push_back(e21);
    featOf.push_back(i);
  }
  const int nCorr = (int)featOf.size();
  P.active.assign(P.edges.size(), 1);
  int it1 = 0, tr1 = 0, it2 = 0, tr2 = 0;
  if (nCorr > 0) optimize(P, 5, &it1, &tr1);
  int nBad = 0;
  for (int c = 0; c < nCorr; ++c) {
    Edge& a = P.edges[2 * c];
    Edge& b = P.edges[2 * c + 1];
    if (Problem::chi2(a) > th2 || Problem::chi2(b) > th2) {
      keep[featOf[c]] = 0;
      P.active[2 * c] = P.active[2 * c + 1] = 0;
      nBad++;
      continue;
    }
    a.robust = b.robust = false;
  }
  const int nMore = nBad > 0 ? 10 : 5;
  stats[0] = it1; stats[1] = tr1; stats[5] = nCorr; stats[6] = nBad;
  if (nCorr - nBad < 10) {
    stats[2] = stats[3] = stats[4] = stats[7] = 0;
    return 0;
  }
  optimize(P, nMore, &it2, &tr2);
  int nIn = 0;
  for (int c = 0; c < nCorr; ++c) {
    if (!P.active[2 * c]) continue;
    Edge& a = P.edges[2 * c];
    Edge& b = P.edges[2 * c + 1];
    P.computeError(a, P.est);
    P.computeError(b, P.est);
    if (Problem::chi2(a) > th2 || Problem::chi2(b) > th2) keep[featOf[c]] = 0;
    else nIn++;
  }
  for (int k = 0; k < 4; ++k) S12[k] = P.est.q[k];
  for (int k = 0; k < 3; ++k) S12[4 + k] = P.est.t[k];
  S12[7] = P.est.s;
  stats[2] = it2; stats[3] = tr2; stats[4] = 1; stats[7] = nIn;
  return nIn;
}

}  // extern "C"
