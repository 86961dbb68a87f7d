// CPU oracle of Optimizer::OptimizeEssentialGraph4DoF on the flattened graph (include/morb_hip.h: morb_optimize_essential_graph_4dof): an
// Eigen-free FP64 restatement of VertexPose4DoF / ImuCamPose::UpdateW (G2oTypes.h:155-189, G2oTypes.cc:218-248, with the counter of five
// updates and the four zeroed entries of DR), Edge4DoF (G2oTypes.h:816-842), ExpSO3 / LogSO3 (G2oTypes.cc:783-811), the numeric Jacobians of
// BaseBinaryEdge::linearizeOplus (central differences, delta = 1e-9, on a pushed copy), constructQuadraticForm's non-robust branch with the
// information diag(1e3, 1e3, 1, 1, 1, 1), g2o's Levenberg-Marquardt (lambda from computeLambdaInit: 1e-5 * max |H_jj|; optimize(20)) and the
// point correction of Optimizer.cc:5451-5470.  The linear system is solved by a plain scalar skyline LDL^T (row envelopes), written
// independently of the library's block-column schedule.  NormalizeRotation (U V^T of the SVD) is the polar factor, taken by Newton's
// iteration; the rotation matrix -> quaternion -> rotation round trip of g2o::Sim3(Ri, ti, 1.) in the point correction is left out (it
// moves a point by rounding).
// -DPG4_ORACLE_REVERSE: the edges are visited in reverse wherever a sum runs over them (the second build of the tests).
// -DPG4_ORACLE_NUDGE: acos and sin inside LogSO3 land one ulp towards zero; -DPG4_ORACLE_JITTER=k: the matrix entries a few ulp off before
// the factorisation (further builds, for the corpus selection).
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

#ifdef PG4_ORACLE_NUDGE
double acos_(double x) { return nextafter(acos(x), 0.0); }
double sin_(double x) { return nextafter(sin(x), 0.0); }
#else
double acos_(double x) { return acos(x); }
double sin_(double x) { return sin(x); }
#endif

struct M3 { double m[9]; };
M3 mul(const M3& a, const M3& b) {
  M3 r;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r.m[i * 3 + j] = a.m[i * 3] * b.m[j] + a.m[i * 3 + 1] * b.m[3 + j] + a.m[i * 3 + 2] * b.m[6 + j];
  return r;
}
M3 tr(const M3& a) {
  M3 r;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r.m[i * 3 + j] = a.m[j * 3 + i];
  return r;
}
void mulv(const M3& a, const double* v, double* o) {
  double t[3];
  for (int i = 0; i < 3; ++i) t[i] = a.m[i * 3] * v[0] + a.m[i * 3 + 1] * v[1] + a.m[i * 3 + 2] * v[2];
  for (int i = 0; i < 3; ++i) o[i] = t[i];
}
M3 identity() { M3 r; for (int k = 0; k < 9; ++k) r.m[k] = (k % 4 == 0) ? 1.0 : 0.0; return r; }

// NormalizeRotation: U V^T of the SVD = the orthogonal polar factor; X <- (X + X^-T) / 2 converges quadratically from a near-rotation
M3 normalize_rotation(const M3& R) {
  M3 X = R;
  for (int it = 0; it < 3; ++it) {
    const double* x = X.m;
    const double c[9] = {x[4] * x[8] - x[5] * x[7], x[5] * x[6] - x[3] * x[8], x[3] * x[7] - x[4] * x[6],
                         x[2] * x[7] - x[1] * x[8], x[0] * x[8] - x[2] * x[6], x[1] * x[6] - x[0] * x[7],
                         x[1] * x[5] - x[2] * x[4], x[2] * x[3] - x[0] * x[5], x[0] * x[4] - x[1] * x[3]};
    const double inv = 1.0 / (x[0] * c[0] + x[1] * c[1] + x[2] * c[2]);
    M3 Y;
    for (int k = 0; k < 9; ++k) Y.m[k] = 0.5 * (x[k] + c[k] * inv);
    X = Y;
  }
  return X;
}
M3 exp_so3(double x, double y, double z) {   // G2oTypes.cc:783-796
  const double d2 = x * x + y * y + z * z, d = sqrt(d2);
  const M3 W = {{0.0, -z, y, z, 0.0, -x, -y, x, 0.0}};
  const M3 WW = mul(W, W);
  M3 res = identity();
  if (d < 1e-5) {
    for (int k = 0; k < 9; ++k) res.m[k] += W.m[k] + 0.5 * WW.m[k];
  } else {
    for (int k = 0; k < 9; ++k) res.m[k] += W.m[k] * sin(d) / d + WW.m[k] * (1.0 - cos(d)) / d2;
  }
  return normalize_rotation(res);
}
void log_so3(const M3& R, double* w) {   // G2oTypes.cc:798-811
  const double t = R.m[0] + R.m[4] + R.m[8];
  w[0] = (R.m[7] - R.m[5]) / 2; w[1] = (R.m[2] - R.m[6]) / 2; w[2] = (R.m[3] - R.m[1]) / 2;
  const double costheta = (t - 1.0) * 0.5f;
  if (costheta > 1 || costheta < -1) return;
  const double theta = acos_(costheta);
  const double s = sin_(theta);
  if (fabs(s) < 1e-5) return;
  for (int k = 0; k < 3; ++k) w[k] = theta * w[k] / s;
}

struct Calib { M3 Rcb; double tcb[3]; };
struct Vertex {   // ImuCamPose, what the 4-DoF graph touches
  M3 Rcw, Rwb0, DR;
  double tcw[3], twb[3];
  int its;
};
void update_w(Vertex& v, const Calib& K, const double* u4) {   // VertexPose4DoF::oplusImpl -> ImuCamPose::UpdateW
  const M3 dR = exp_so3(0.0, 0.0, u4[0]);
  v.DR = mul(dR, v.DR);
  const M3 Rwb = mul(v.DR, v.Rwb0);
  for (int k = 0; k < 3; ++k) v.twb[k] += u4[1 + k];
  v.its++;
  if (v.its >= 5) {
    v.DR.m[2] = 0.0; v.DR.m[5] = 0.0; v.DR.m[6] = 0.0; v.DR.m[7] = 0.0;
    (void)normalize_rotation(v.DR);   // (the reference discards the result as well)
    v.its = 0;
  }
  const M3 Rbw = tr(Rwb);
  double tbw[3];
  mulv(Rbw, v.twb, tbw);
  for (int k = 0; k < 3; ++k) tbw[k] = -tbw[k];
  v.Rcw = mul(K.Rcb, Rbw);
  mulv(K.Rcb, tbw, v.tcw);
  for (int k = 0; k < 3; ++k) v.tcw[k] += K.tcb[k];
}
struct Meas { M3 dR; double dt[3]; };
void edge_error(const Meas& M, const Vertex& Vi, const Vertex& Vj, double* e) {   // Edge4DoF::computeError
  const M3 RjT = tr(Vj.Rcw);
  log_so3(mul(mul(Vi.Rcw, RjT), tr(M.dR)), e);
  double v[3];
  mulv(RjT, Vj.tcw, v);
  for (int k = 0; k < 3; ++k) v[k] = -v[k];
  mulv(Vi.Rcw, v, v);
  for (int k = 0; k < 3; ++k) e[3 + k] = v[k] + Vi.tcw[k] - M.dt[k];
}
const double OMEGA[6] = {1e3, 1e3, 1, 1, 1, 1};
double chi2_of(const double* e) {
  double c = 0;
  for (int k = 0; k < 6; ++k) c += e[k] * (OMEGA[k] * e[k]);
  return c;
}

struct Graph {
  int nKF, nE, n;
  const uint8_t* fixed;
  const int *eI, *eJ;
  Calib K;
  std::vector<Meas> M;
  std::vector<Vertex> V;
  std::vector<int> col;          // vertex -> block row, or -1
  std::vector<int> first;        // scalar row -> first scalar column of its envelope
  std::vector<std::vector<double>> H;   // scalar rows over their envelopes
  std::vector<double> b;
  std::vector<double> J;         // [nE][2][24]
  std::vector<double> err;       // [nE][6]
};

template <class F>
void for_edges(int nE, F&& f) {
#ifdef PG4_ORACLE_REVERSE
  for (int e = nE - 1; e >= 0; --e) f(e);
#else
  for (int e = 0; e < nE; ++e) f(e);
#endif
}

double active_chi2(const Graph& g, const std::vector<Vertex>& X) {
  double chi = 0;
  for_edges(g.nE, [&](int e) {
    double er[6];
    edge_error(g.M[e], X[g.eI[e]], X[g.eJ[e]], er);
    chi += chi2_of(er);
  });
  return chi;
}

void linearize(Graph& g) {
  const double delta = 1e-9, scalar = 1.0 / (2 * delta);
  for (int e = 0; e < g.nE; ++e) {
    const Vertex &Vi = g.V[g.eI[e]], &Vj = g.V[g.eJ[e]];
    edge_error(g.M[e], Vi, Vj, &g.err[(size_t)e * 6]);
    for (int side = 0; side < 2; ++side) {
      const int v = side ? g.eJ[e] : g.eI[e];
      if (g.fixed[v]) continue;
      double* J = &g.J[((size_t)e * 2 + side) * 24];
      for (int d = 0; d < 4; ++d) {
        double add[4] = {0, 0, 0, 0}, ep[6], em[6];
        Vertex P = g.V[v], Q = g.V[v];   // push
        add[d] = delta;
        update_w(P, g.K, add);
        add[d] = -delta;
        update_w(Q, g.K, add);
        if (side) { edge_error(g.M[e], Vi, P, ep); edge_error(g.M[e], Vi, Q, em); }
        else { edge_error(g.M[e], P, Vj, ep); edge_error(g.M[e], Q, Vj, em); }
        for (int r = 0; r < 6; ++r) J[r * 4 + d] = scalar * (ep[r] - em[r]);
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
    const double *Ji = &g.J[((size_t)e * 2) * 24], *Jj = &g.J[((size_t)e * 2 + 1) * 24], *er = &g.err[(size_t)e * 6];
    for (int side = 0; side < 2; ++side) {
      const int blk = side ? bcol : a;
      if (blk < 0) continue;
      const double* Jx = side ? Jj : Ji;
      for (int r = 0; r < 4; ++r) {
        double v = 0;
        for (int k = 0; k < 6; ++k) v += Jx[k * 4 + r] * (-(OMEGA[k] * er[k]));
        g.b[blk * 4 + r] += v;
        for (int c = 0; c <= r; ++c) {
          double h = 0;
          for (int k = 0; k < 6; ++k) h += (Jx[k * 4 + r] * OMEGA[k]) * Jx[k * 4 + c];
          at(blk * 4 + r, blk * 4 + c) += h;
        }
      }
    }
    if (a >= 0 && bcol >= 0) {
      const double *Jr = a > bcol ? Ji : Jj, *Jc = a > bcol ? Jj : Ji;
      const int br = a > bcol ? a : bcol, bc = a > bcol ? bcol : a;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
          double h = 0;
          for (int k = 0; k < 6; ++k) h += (Jr[k * 4 + r] * OMEGA[k]) * Jc[k * 4 + c];
          at(br * 4 + r, bc * 4 + c) += h;
        }
    }
  });
}

// (H + lambda I) x = b by a scalar skyline LDL^T; false: a pivot is not positive
bool solve(const Graph& g, double lambda, std::vector<double>& x) {
  const int N = 4 * g.n;
  std::vector<std::vector<double>> L(g.H);
  std::vector<double> d(N);
  for (int i = 0; i < N; ++i) {
    const int fi = g.first[i];
    L[i][i - fi] += lambda;
#ifdef PG4_ORACLE_JITTER   // (= 0, 1, ...: the pattern) every entry off by up to three ulp: what another elimination schedule's rounding does to the matrix
    for (int j = fi; j <= i; ++j) L[i][j - fi] *= (1 + 2.2e-16 * (((i * 31 + j * 17 + PG4_ORACLE_JITTER) % 7) - 3));
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

double max_diagonal(const Graph& g) {   // computeLambdaInit's loop
  double m = 0;
  for (int i = 0; i < 4 * g.n; ++i) m = std::fmax(std::fabs(g.H[i][i - g.first[i]]), m);
  return m;
}

void setup(Graph& g, int nKF, const double* pose, const double* body, const uint8_t* fixed, const float* Tcb12, int nE, const int* eI, const int* eJ,
           const double* eT) {
  g.nKF = nKF; g.nE = nE; g.fixed = fixed; g.eI = eI; g.eJ = eJ;
  for (int k = 0; k < 9; ++k) g.K.Rcb.m[k] = (double)Tcb12[k];
  for (int k = 0; k < 3; ++k) g.K.tcb[k] = (double)Tcb12[9 + k];
  g.V.resize(nKF);
  for (int v = 0; v < nKF; ++v) {
    Vertex& V = g.V[v];
    memcpy(V.Rcw.m, pose + (size_t)v * 12, sizeof(double) * 9); memcpy(V.tcw, pose + (size_t)v * 12 + 9, sizeof(double) * 3);
    memcpy(V.Rwb0.m, body + (size_t)v * 12, sizeof(double) * 9); memcpy(V.twb, body + (size_t)v * 12 + 9, sizeof(double) * 3);
    V.DR = identity();
    V.its = 0;
  }
  g.M.resize(nE);
  for (int e = 0; e < nE; ++e) { memcpy(g.M[e].dR.m, eT + (size_t)e * 12, sizeof(double) * 9); memcpy(g.M[e].dt, eT + (size_t)e * 12 + 9, sizeof(double) * 3); }
  std::vector<char> used(nKF, 0);
  for (int e = 0; e < nE; ++e) used[eI[e]] = used[eJ[e]] = 1;
  g.col.assign(nKF, -1);
  g.n = 0;
  for (int v = 0; v < nKF; ++v) if (!fixed[v] && used[v]) g.col[v] = g.n++;
  std::vector<int> bf(g.n);
  for (int r = 0; r < g.n; ++r) bf[r] = r;
  for (int e = 0; e < nE; ++e) {
    const int a = g.col[eI[e]], b = g.col[eJ[e]];
    if (a >= 0 && b >= 0) { const int hi = a > b ? a : b, lo = a > b ? b : a; if (lo < bf[hi]) bf[hi] = lo; }
  }
  g.first.resize(4 * g.n); g.H.resize(4 * g.n); g.b.assign(4 * g.n, 0.0);
  for (int i = 0; i < 4 * g.n; ++i) { g.first[i] = 4 * bf[i / 4]; g.H[i].assign(i - g.first[i] + 1, 0.0); }
  g.J.assign((size_t)nE * 48, 0.0); g.err.assign((size_t)nE * 6, 0.0);
}

void q_rotate(const double* q, const double* v, double* o) {   // QuaternionBase::_transformVector
  const double ux = q[0], uy = q[1], uz = q[2], w = q[3];
  double a = uy * v[2] - uz * v[1], b = uz * v[0] - ux * v[2], c = ux * v[1] - uy * v[0];
  a += a; b += b; c += c;
  o[0] = v[0] + w * a + (uy * c - uz * b);
  o[1] = v[1] + w * b + (uz * a - ux * c);
  o[2] = v[2] + w * c + (ux * b - uy * a);
}

}  // namespace

extern "C" {

// Edge4DoF::computeError on two camera poses (12 doubles each: R row-major, t) and a measurement (12 doubles): e[6]
void pg4_oracle_error(const double* Pi, const double* Pj, const double* T, double* e6) {
  Vertex a, b;
  Meas M;
  memcpy(a.Rcw.m, Pi, sizeof(double) * 9); memcpy(a.tcw, Pi + 9, sizeof(double) * 3);
  memcpy(b.Rcw.m, Pj, sizeof(double) * 9); memcpy(b.tcw, Pj + 9, sizeof(double) * 3);
  memcpy(M.dR.m, T, sizeof(double) * 9); memcpy(M.dt, T + 9, sizeof(double) * 3);
  edge_error(M, a, b, e6);
}
// VertexPose4DoF::oplusImpl on a fresh vertex (DR = I, its = 0): the camera pose (12 doubles) after the update u4
void pg4_oracle_oplus(const double* body12, const float* Tcb12, const double* u4, double* pose12) {
  Calib K;
  for (int k = 0; k < 9; ++k) K.Rcb.m[k] = (double)Tcb12[k];
  for (int k = 0; k < 3; ++k) K.tcb[k] = (double)Tcb12[9 + k];
  Vertex V;
  memcpy(V.Rwb0.m, body12, sizeof(double) * 9); memcpy(V.twb, body12 + 9, sizeof(double) * 3);
  V.DR = identity(); V.its = 0;
  update_w(V, K, u4);
  memcpy(pose12, V.Rcw.m, sizeof(double) * 9); memcpy(pose12 + 9, V.tcw, sizeof(double) * 3);
}

// the quadratic form at the entry states as a dense symmetric matrix Hd [4n][4n] and bd [4n], the solution xd [4n] of (H + lambda I) x = b by
// the envelope solve (ok[0] = it succeeded), and the Jacobians Jd [nE][2][24]; returns n
int pg4_oracle_system(int nKF, const double* pose, const double* body, const uint8_t* fixed, const float* Tcb12, int nE, const int* eI, const int* eJ,
                      const double* eT, double lambda, double* Hd, double* bd, double* xd, int* ok, double* Jd) {
  Graph g;
  setup(g, nKF, pose, body, fixed, Tcb12, nE, eI, eJ, eT);
  if (!Hd) return g.n;
  linearize(g);
  build(g);
  const int N = 4 * g.n;
  for (int i = 0; i < N * N; ++i) Hd[i] = 0;
  for (int i = 0; i < N; ++i)
    for (int j = g.first[i]; j <= i; ++j) Hd[i * N + j] = Hd[j * N + i] = g.H[i][j - g.first[i]];
  for (int i = 0; i < N; ++i) bd[i] = g.b[i];
  std::vector<double> x(N, 0.0);
  ok[0] = solve(g, lambda, x) ? 1 : 0;
  for (int i = 0; i < N; ++i) xd[i] = x[i];
  if (Jd) memcpy(Jd, g.J.data(), sizeof(double) * g.J.size());
  return g.n;
}

// the whole call: the poses in place, the points in place, stats4 = {outer iterations, trials, vertices in the system, envelope blocks},
// chi2[2], accepted = the number of accepted steps
void pg4_oracle_run(int nKF, double* pose, const double* body, const uint8_t* fixed, const float* Tcb12, int nE, const int* eI, const int* eJ,
                    const double* eT, int nMP, float* mp, const int* mpRef, const double* Scw, int* stats4, double* chi2, int* accepted) {
  Graph g;
  setup(g, nKF, pose, body, fixed, Tcb12, nE, eI, eJ, eT);
  for (int k = 0; k < 4; ++k) stats4[k] = 0;
  chi2[0] = chi2[1] = 0;
  *accepted = 0;
  if (!g.n) return;
  int blocks = 0;
  for (int r = 0; r < g.n; ++r) blocks += r - g.first[4 * r] / 4 + 1;
  stats4[2] = g.n; stats4[3] = blocks;
  // OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:61-169) under SparseOptimizer::optimize(20)
  std::vector<double> x(4 * g.n, 0.0);
  double lambda = 0, ni = 2, currentChi = active_chi2(g, g.V);
  chi2[0] = currentChi;
  int nBad = 0, its = 0, trials = 0;
  for (int it = 0; it < 20; ++it) {
    linearize(g);
    build(g);
    const double iniChi = currentChi;
    if (it == 0) { lambda = 1e-5 * max_diagonal(g); ni = 2; nBad = 0; }   // computeLambdaInit
    double rho = 0;
    int qmax = 0;
    do {
      const bool ok2 = solve(g, lambda, x);
      std::vector<Vertex> T(g.V);   // push
      for (int v = 0; v < nKF; ++v) if (g.col[v] >= 0) update_w(T[v], g.K, &x[g.col[v] * 4]);
      double tempChi = active_chi2(g, T);
      if (!ok2) tempChi = DBL_MAX;
      rho = (currentChi - tempChi);
      double scale = 0;
      for (int j = 0; j < 4 * g.n; ++j) scale += x[j] * (lambda * x[j] + g.b[j]);
      scale += 1e-3;
      rho /= scale;
      if (rho > 0 && std::isfinite(tempChi)) {
        double alpha = 1. - pow(2 * rho - 1, 3);
        alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
        const double scaleFactor = 1. / 3. > alpha ? 1. / 3. : alpha;
        lambda *= scaleFactor;
        ni = 2;
        currentChi = tempChi;
        g.V = T;   // discardTop
        ++*accepted;
      } else {
        lambda *= ni;   // pop
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
  for (int v = 0; v < nKF; ++v) { memcpy(pose + (size_t)v * 12, g.V[v].Rcw.m, sizeof(double) * 9); memcpy(pose + (size_t)v * 12 + 9, g.V[v].tcw, sizeof(double) * 3); }
  for (int m = 0; m < nMP; ++m) {
    const int v = mpRef[m];
    if (v < 0) continue;
    const double* S = Scw + (size_t)v * 8;
    const double P[3] = {(double)mp[m * 3], (double)mp[m * 3 + 1], (double)mp[m * 3 + 2]};
    double a[3], o[3];
    q_rotate(S, P, a);
    for (int k = 0; k < 3; ++k) a[k] = S[7] * a[k] + S[4 + k] - g.V[v].tcw[k];   // Srw.map(P), then the inverse of (Ri, ti, 1)
    mulv(tr(g.V[v].Rcw), a, o);
    for (int k = 0; k < 3; ++k) mp[m * 3 + k] = (float)o[k];
  }
}

}
