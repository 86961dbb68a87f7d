// CPU oracle of Optimizer::InertialOptimization (reference src/Optimizer.cc:2979-3428) for the tests: an independent restatement written
// from the reference's behaviour — EdgeInertialGS (G2oTypes.cc:587-727), the bias priors, VertexGDir / VertexScale, g2o's
// Levenberg-Marquardt with ORB-SLAM's stop rule and g2o's Gauss-Newton — on a DENSE system with a plain dense LDL^T.  It shares no code
// with the kernel or with include/morb/arrowhead_math.h.  Built by tests/inertial_optimization_oracle.py (g++ -O2 -ffp-contract=off; a
// second way, -O3 -ffp-contract=fast with IO_ORACLE_REVERSE, for the corpus-selection test: the links are then summed in reverse order).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

namespace {

struct Preint {   // morb_imu_preintegrated, field by field
  float dT, dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], C[225], b[6], nga[6], ngaWalk[6], avgA[3], avgW[3];
};
static_assert(sizeof(Preint) == 4 * 310, "310 floats");

const double GRAV = (double)9.81f;

void mm(const double* A, const double* B, double* C) {
  double t[9];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) t[r * 3 + c] = A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c] + A[r * 3 + 2] * B[6 + c];
  memcpy(C, t, sizeof t);
}
void mv(const double* A, const double* v, double* o) {
  double t[3];
  for (int r = 0; r < 3; ++r) t[r] = A[r * 3] * v[0] + A[r * 3 + 1] * v[1] + A[r * 3 + 2] * v[2];
  memcpy(o, t, sizeof t);
}
void tr(const double* A, double* T) {
  double t[9];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) t[r * 3 + c] = A[c * 3 + r];
  memcpy(T, t, sizeof t);
}
void hat(const double* v, double* W) { W[0] = 0; W[1] = -v[2]; W[2] = v[1]; W[3] = v[2]; W[4] = 0; W[5] = -v[0]; W[6] = -v[1]; W[7] = v[0]; W[8] = 0; }
const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

void ExpSO3(double x, double y, double z, double* R) {
  const double d2 = x * x + y * y + z * z, d = std::sqrt(d2);
  const double v[3] = {x, y, z};
  double W[9], WW[9];
  hat(v, W); mm(W, W, WW);
  if (d < 1e-5) for (int k = 0; k < 9; ++k) R[k] = I3[k] + W[k] + 0.5 * WW[k];
  else for (int k = 0; k < 9; ++k) R[k] = I3[k] + W[k] * std::sin(d) / d + WW[k] * (1.0 - std::cos(d)) / d2;
}
void LogSO3(const double* R, double* w) {
  const double t = R[0] + R[4] + R[8];
  w[0] = (R[7] - R[5]) / 2; w[1] = (R[2] - R[6]) / 2; w[2] = (R[3] - R[1]) / 2;
  const double costheta = (t - 1.0) * 0.5f;
  if (costheta > 1 || costheta < -1) return;
  const double theta = std::acos(costheta), s = std::sin(theta);
  if (std::fabs(s) < 1e-5) return;
  for (int k = 0; k < 3; ++k) w[k] = theta * w[k] / s;
}
void InverseRightJacobianSO3(const double* v, double* J) {
  const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], d = std::sqrt(d2);
  double W[9], WW[9];
  hat(v, W); mm(W, W, WW);
  if (d < 1e-5) { memcpy(J, I3, sizeof I3); return; }
  for (int k = 0; k < 9; ++k) J[k] = I3[k] + W[k] / 2 + WW[k] * (1.0 / d2 - (1.0 + std::cos(d)) / (2.0 * d * std::sin(d)));
}
void RightJacobianSO3(const double* v, double* J) {
  const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], d = std::sqrt(d2);
  double W[9], WW[9];
  hat(v, W); mm(W, W, WW);
  if (d < 1e-5) { memcpy(J, I3, sizeof I3); return; }
  for (int k = 0; k < 9; ++k) J[k] = I3[k] - W[k] * (1.0 - std::cos(d)) / d2 + WW[k] * (d - std::sin(d)) / (d2 * d);
}

// NormalizeRotation (ImuTypes.cc:35-39): U V^T of the SVD = the orthogonal polar factor, here by Newton's iteration in double
void NormalizeRotation(float* R) {
  double X[9];
  for (int k = 0; k < 9; ++k) X[k] = R[k];
  for (int it = 0; it < 4; ++it) {
    const double det = X[0] * (X[4] * X[8] - X[5] * X[7]) - X[1] * (X[3] * X[8] - X[5] * X[6]) + X[2] * (X[3] * X[7] - X[4] * X[6]);
    const double invT[9] = {(X[4] * X[8] - X[5] * X[7]) / det, (X[5] * X[6] - X[3] * X[8]) / det, (X[3] * X[7] - X[4] * X[6]) / det,
                            (X[2] * X[7] - X[1] * X[8]) / det, (X[0] * X[8] - X[2] * X[6]) / det, (X[1] * X[6] - X[0] * X[7]) / det,
                            (X[1] * X[5] - X[2] * X[4]) / det, (X[2] * X[3] - X[0] * X[5]) / det, (X[0] * X[4] - X[1] * X[3]) / det};
    for (int k = 0; k < 9; ++k) X[k] = 0.5 * (X[k] + invT[k]);
  }
  for (int k = 0; k < 9; ++k) R[k] = (float)X[k];
}
void mmf(const float* A, const float* B, float* C) {
  float t[9];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) t[r * 3 + c] = A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c] + A[r * 3 + 2] * B[6 + c];
  memcpy(C, t, sizeof t);
}
void mvf(const float* A, const float* v, float* o) {
  for (int r = 0; r < 3; ++r) o[r] = A[r * 3] * v[0] + A[r * 3 + 1] * v[1] + A[r * 3 + 2] * v[2];
}
// GetDeltaRotation / GetDeltaVelocity / GetDeltaPosition / GetDeltaBias at the bias (bg, ba): float arithmetic (ImuTypes.cc:289-312)
void Deltas(const Preint& P, const double* bg, const double* ba, double* dR, double* dV, double* dP, double* dbgOut) {
  const float dbg[3] = {(float)bg[0] - P.b[3], (float)bg[1] - P.b[4], (float)bg[2] - P.b[5]};
  const float dba[3] = {(float)ba[0] - P.b[0], (float)ba[1] - P.b[1], (float)ba[2] - P.b[2]};
  float w[3];
  mvf(P.JRg, dbg, w);
  const float d2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], d = std::sqrt(d2);
  const float W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  float WW[9], E[9], R[9];
  mmf(W, W, WW);
  const float If[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (d < 1e-5f) for (int k = 0; k < 9; ++k) E[k] = If[k] + W[k] + 0.5f * WW[k];
  else for (int k = 0; k < 9; ++k) E[k] = If[k] + W[k] * std::sin(d) / d + WW[k] * (1.0f - std::cos(d)) / d2;
  mmf(P.dR, E, R);
  NormalizeRotation(R);
  for (int k = 0; k < 9; ++k) dR[k] = R[k];
  float a[3], b[3];
  mvf(P.JVg, dbg, a); mvf(P.JVa, dba, b);
  for (int k = 0; k < 3; ++k) dV[k] = (double)(P.dV[k] + a[k] + b[k]);
  mvf(P.JPg, dbg, a); mvf(P.JPa, dba, b);
  for (int k = 0; k < 3; ++k) dP[k] = (double)(P.dP[k] + a[k] + b[k]);
  for (int k = 0; k < 3; ++k) dbgOut[k] = dbg[k];
}

struct Globals { double Rwg[9], s, bg[3], ba[3]; };

// computeError and (J != null) linearizeOplus: J is 9 x 15, columns velocity 1 (0..2), velocity 2 (3..5), gyro bias (6..8), acc bias (9..11),
// gravity direction (12, 13), scale (14)
void Edge(const Preint& P, const float* s1, const float* s2, const double* v1, const double* v2, const Globals& G, double* e, double* J) {
  double dR[9], dV[3], dP[3], dbg[3], Rwb1[9], Rwb2[9], Rbw1[9], dRt[9], eR[9], er[3];
  Deltas(P, G.bg, G.ba, dR, dV, dP, dbg);
  for (int k = 0; k < 9; ++k) { Rwb1[k] = s1[k]; Rwb2[k] = s2[k]; }
  tr(Rwb1, Rbw1); tr(dR, dRt);
  mm(dRt, Rbw1, eR); mm(eR, Rwb2, eR);
  LogSO3(eR, er);
  const double dt = P.dT, s = G.s;
  const double g[3] = {G.Rwg[2] * -GRAV, G.Rwg[5] * -GRAV, G.Rwg[8] * -GRAV};
  double dv[3], dp[3], t[3], ev[3], ep[3];
  for (int k = 0; k < 3; ++k) { dv[k] = v2[k] - v1[k]; dp[k] = (double)s2[9 + k] - (double)s1[9 + k] - v1[k] * dt; }
  for (int k = 0; k < 3; ++k) t[k] = s * dv[k] - g[k] * dt;
  mv(Rbw1, t, ev);
  for (int k = 0; k < 3; ++k) t[k] = s * dp[k] - g[k] * dt * dt / 2;
  mv(Rbw1, t, ep);
  for (int k = 0; k < 3; ++k) { e[k] = er[k]; e[3 + k] = ev[k] - dV[k]; e[6 + k] = ep[k] - dP[k]; }
  if (!J) return;
  for (int k = 0; k < 135; ++k) J[k] = 0;
  auto put = [&](int r0, int c0, const double* B, double f) { for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) J[(r0 + r) * 15 + c0 + c] = f * B[r * 3 + c]; };
  put(3, 0, Rbw1, -s); put(6, 0, Rbw1, -s * dt);      // velocity 1
  put(3, 3, Rbw1, s);                                  // velocity 2
  double invJr[9], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], w3[3], rj[9], eRt[9], T[9];
  for (int k = 0; k < 9; ++k) { JRg[k] = P.JRg[k]; JVg[k] = P.JVg[k]; JVa[k] = P.JVa[k]; JPg[k] = P.JPg[k]; JPa[k] = P.JPa[k]; }
  InverseRightJacobianSO3(er, invJr);
  mv(JRg, dbg, w3);
  RightJacobianSO3(w3, rj);
  tr(eR, eRt);
  mm(invJr, eRt, T); mm(T, rj, T); mm(T, JRg, T);
  put(0, 6, T, -1); put(3, 6, JVg, -1); put(6, 6, JPg, -1);
  put(3, 9, JVa, -1); put(6, 9, JPa, -1);
  // dGdTheta = Rwg * Gm, Gm = [0 -G; G 0; 0 0]
  double dG[6];
  for (int r = 0; r < 3; ++r) { dG[r * 2] = G.Rwg[r * 3 + 1] * GRAV; dG[r * 2 + 1] = G.Rwg[r * 3] * -GRAV; }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 2; ++c) {
      const double v = Rbw1[r * 3] * dG[c] + Rbw1[r * 3 + 1] * dG[2 + c] + Rbw1[r * 3 + 2] * dG[4 + c];
      J[(3 + r) * 15 + 12 + c] = -v * dt;
      J[(6 + r) * 15 + 12 + c] = -0.5 * v * dt * dt;
    }
  double a[3], b[3];
  mv(Rbw1, dv, a); mv(Rbw1, dp, b);
  for (int r = 0; r < 3; ++r) { J[(3 + r) * 15 + 14] = a[r]; J[(6 + r) * 15 + 14] = b[r]; }
}

// dense inverse by Gauss-Jordan with partial pivoting
bool Inverse(int n, const double* A, double* Ai) {
  std::vector<double> M(n * 2 * n);
  for (int r = 0; r < n; ++r) for (int c = 0; c < 2 * n; ++c) M[r * 2 * n + c] = c < n ? A[r * n + c] : (c - n == r ? 1.0 : 0.0);
  for (int c = 0; c < n; ++c) {
    int p = c;
    for (int r = c + 1; r < n; ++r) if (std::fabs(M[r * 2 * n + c]) > std::fabs(M[p * 2 * n + c])) p = r;
    if (M[p * 2 * n + c] == 0.0) return false;
    if (p != c) for (int k = 0; k < 2 * n; ++k) std::swap(M[p * 2 * n + k], M[c * 2 * n + k]);
    const double inv = 1.0 / M[c * 2 * n + c];
    for (int k = 0; k < 2 * n; ++k) M[c * 2 * n + k] *= inv;
    for (int r = 0; r < n; ++r) {
      if (r == c) continue;
      const double f = M[r * 2 * n + c];
      if (f != 0.0) for (int k = 0; k < 2 * n; ++k) M[r * 2 * n + k] -= f * M[c * 2 * n + k];
    }
  }
  for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) Ai[r * n + c] = M[r * 2 * n + n + c];
  return true;
}
// symmetric eigen-decomposition by cyclic Jacobi: A = V diag(e) V^T
void Eigen9(const double* S, double* e, double* V) {
  double A[81];
  memcpy(A, S, sizeof A);
  for (int k = 0; k < 81; ++k) V[k] = (k % 10 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 80; ++sweep) {
    double off = 0, diag = 0;
    for (int r = 0; r < 9; ++r) for (int c = 0; c < 9; ++c) { const double t = A[r * 9 + c] * A[r * 9 + c]; if (r == c) diag += t; else off += t; }
    if (off <= 1e-32 * diag) break;
    for (int p = 0; p < 9; ++p)
      for (int q = p + 1; q < 9; ++q) {
        if (A[p * 9 + q] == 0.0) continue;
        const double th = (A[q * 9 + q] - A[p * 9 + p]) / (2.0 * A[p * 9 + q]);
        const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 9; ++k) { const double a = A[k * 9 + p], b = A[k * 9 + q]; A[k * 9 + p] = c * a - s * b; A[k * 9 + q] = s * a + c * b; }
        for (int k = 0; k < 9; ++k) { const double a = A[p * 9 + k], b = A[q * 9 + k]; A[p * 9 + k] = c * a - s * b; A[q * 9 + k] = s * a + c * b; }
        for (int k = 0; k < 9; ++k) { const double a = V[k * 9 + p], b = V[k * 9 + q]; V[k * 9 + p] = c * a - s * b; V[k * 9 + q] = s * a + c * b; }
      }
  }
  for (int k = 0; k < 9; ++k) e[k] = A[k * 9 + k];
}
// EdgeInertialGS's information: inverse of C(0:9, 0:9), symmetrised, eigenvalues below 1e-12 zeroed
void Information(const Preint& P, double* Info) {
  double C9[81];
  for (int r = 0; r < 9; ++r) for (int c = 0; c < 9; ++c) C9[r * 9 + c] = (double)P.C[r * 15 + c];
  if (!Inverse(9, C9, Info)) { for (int k = 0; k < 81; ++k) Info[k] = 0; return; }
  for (int r = 0; r < 9; ++r) for (int c = r + 1; c < 9; ++c) { const double s = (Info[r * 9 + c] + Info[c * 9 + r]) / 2; Info[r * 9 + c] = s; Info[c * 9 + r] = s; }
  double e[9], V[81];
  Eigen9(Info, e, V);
  bool any = false;
  for (int k = 0; k < 9; ++k) if (e[k] < 1e-12) { e[k] = 0; any = true; }
  if (!any) return;   // V diag(e) V^T with no eigenvalue changed is Info itself up to rounding
  for (int r = 0; r < 9; ++r) for (int c = 0; c < 9; ++c) { double s = 0; for (int k = 0; k < 9; ++k) s += V[r * 9 + k] * e[k] * V[c * 9 + k]; Info[r * 9 + c] = s; }
}

// plain dense LDL^T solve; false when a pivot is not positive
bool SolveDense(int m, std::vector<double> A, const std::vector<double>& b, std::vector<double>& x) {
  for (int j = 0; j < m; ++j) {
    const double d = A[(size_t)j * m + j];
    if (!(d > 0)) return false;
    for (int r = j + 1; r < m; ++r) {
      const double a = A[(size_t)r * m + j];
      if (a == 0.0) continue;
      const double l = a / d;
      for (int c = j + 1; c <= r; ++c) A[(size_t)r * m + c] -= l * A[(size_t)c * m + j];
    }
    for (int r = j + 1; r < m; ++r) A[(size_t)r * m + j] /= d;
  }
  std::vector<double> y(b);
  for (int r = 0; r < m; ++r) { double s = y[r]; for (int c = 0; c < r; ++c) s -= A[(size_t)r * m + c] * y[c]; y[r] = s; }
  for (int r = 0; r < m; ++r) y[r] /= A[(size_t)r * m + r];
  for (int r = m - 1; r >= 0; --r) { double s = y[r]; for (int c = r + 1; c < m; ++c) s -= A[(size_t)c * m + r] * y[c]; y[r] = s; }
  x = y;
  return true;
}

struct Problem {
  int n, mode;
  bool freeV, freeB, freeG, freeS, lm;
  const float* st;
  const uint8_t* hl;
  const Preint* P;
  double priorG, priorA;
  std::vector<double> v, Info;
  std::vector<int> link;   // keyframes that carry a link, in summation order
  Globals G;
  int m, ig[9];            // unknowns; index of each global one or -1

  int iv(int k) const { return freeV ? 3 * k : -1; }
  double Chi2() const {
    double tot = 0;
    for (int k : link) {
      double e[9];
      Edge(P[k], st + 21 * (k - 1), st + 21 * k, &v[3 * (k - 1)], &v[3 * k], G, e, nullptr);
      double c = 0;
      for (int r = 0; r < 9; ++r) { double s = 0; for (int l = 0; l < 9; ++l) s += Info[(size_t)k * 81 + r * 9 + l] * e[l]; c += e[r] * s; }
      tot += lm ? c : (c <= 1.0 ? c : 2.0 * std::sqrt(c) - 1.0);
    }
    if (lm) {
      tot += priorA * (G.ba[0] * G.ba[0] + G.ba[1] * G.ba[1] + G.ba[2] * G.ba[2]);
      tot += priorG * (G.bg[0] * G.bg[0] + G.bg[1] * G.bg[1] + G.bg[2] * G.bg[2]);
    }
    return tot;
  }
  void Build(std::vector<double>& H, std::vector<double>& b) const {
    H.assign((size_t)m * m, 0.0); b.assign(m, 0.0);
    for (int k : link) {
      double e[9], J[135], oe[9], OJ[135];
      Edge(P[k], st + 21 * (k - 1), st + 21 * k, &v[3 * (k - 1)], &v[3 * k], G, e, J);
      const double* Om = &Info[(size_t)k * 81];
      double w = 1.0;
      if (!lm) { double c = 0; for (int r = 0; r < 9; ++r) { double s = 0; for (int l = 0; l < 9; ++l) s += Om[r * 9 + l] * e[l]; c += e[r] * s; } w = c <= 1.0 ? 1.0 : 1.0 / std::sqrt(c); }
      for (int r = 0; r < 9; ++r) { double s = 0; for (int l = 0; l < 9; ++l) s += Om[r * 9 + l] * e[l]; oe[r] = w * s; }
      for (int r = 0; r < 9; ++r) for (int c = 0; c < 15; ++c) { double s = 0; for (int l = 0; l < 9; ++l) s += Om[r * 9 + l] * J[l * 15 + c]; OJ[r * 15 + c] = w * s; }
      int idx[15];
      for (int c = 0; c < 3; ++c) { idx[c] = freeV ? 3 * (k - 1) + c : -1; idx[3 + c] = freeV ? 3 * k + c : -1; }
      for (int c = 0; c < 9; ++c) idx[6 + c] = ig[c];
      for (int a = 0; a < 15; ++a) {
        if (idx[a] < 0) continue;
        double s = 0;
        for (int l = 0; l < 9; ++l) s += J[l * 15 + a] * oe[l];
        b[idx[a]] -= s;
        for (int c = 0; c < 15; ++c) {
          if (idx[c] < 0) continue;
          double h = 0;
          for (int l = 0; l < 9; ++l) h += J[l * 15 + a] * OJ[l * 15 + c];
          H[(size_t)idx[a] * m + idx[c]] += h;
        }
      }
    }
    if (lm && freeB) for (int r = 0; r < 3; ++r) {
      H[(size_t)ig[r] * m + ig[r]] += priorG; b[ig[r]] -= priorG * G.bg[r];
      H[(size_t)ig[3 + r] * m + ig[3 + r]] += priorA; b[ig[3 + r]] -= priorA * G.ba[r];
    }
  }
  void Update(const std::vector<double>& x) {
    if (freeV) for (int i = 0; i < 3 * n; ++i) v[i] += x[i];
    if (freeB) for (int r = 0; r < 3; ++r) { G.bg[r] += x[ig[r]]; G.ba[r] += x[ig[3 + r]]; }
    if (freeG) { double dR[9]; ExpSO3(x[ig[6]], x[ig[7]], 0.0, dR); mm(G.Rwg, dR, G.Rwg); }
    if (freeS) G.s = G.s * std::exp(x[ig[8]]);
  }
};

}  // namespace

extern "C" {

// error (9) and Jacobian (9 x 15, columns V1 V2 bg ba gdir scale) of one link; g16 = Rwg, scale, bg, ba
void io_oracle_edge(const float* pre, const float* s1, const float* s2, const double* v1, const double* v2, const double* g16, double* e, double* J) {
  Globals G;
  memcpy(G.Rwg, g16, 72); G.s = g16[9]; memcpy(G.bg, g16 + 10, 24); memcpy(G.ba, g16 + 13, 24);
  Edge(*reinterpret_cast<const Preint*>(pre), s1, s2, v1, v2, G, e, J);
}

// One problem.  kfState [n][21] in / out, hasLink [n], pre [n] records, g16 in / out, reint [n], stats4, chi2 [2].
int io_oracle_run(int n, float* kfState, const uint8_t* hasLink, const float* pre, int mode, int flags, float priorGf, float priorAf, double* g16,
                  uint8_t* reint, int* stats4, double* chi2) {
  Problem Q;
  Q.n = n; Q.mode = mode; Q.st = kfState; Q.hl = hasLink; Q.P = reinterpret_cast<const Preint*>(pre);
  Q.lm = mode != 2;
  Q.freeV = mode == 1 || (mode == 0 && !(flags & 2)); Q.freeB = Q.freeV;
  Q.freeG = mode != 1; Q.freeS = mode == 2 || (mode == 0 && (flags & 1));
  Q.priorG = Q.lm ? (double)priorGf : 0.0; Q.priorA = Q.lm ? (double)priorAf : 0.0;
  for (int k = 1; k < n; ++k) if (hasLink[k]) Q.link.push_back(k);
#ifdef IO_ORACLE_REVERSE
  std::reverse(Q.link.begin(), Q.link.end());
#endif
  stats4[0] = stats4[1] = stats4[2] = 0; stats4[3] = (int)Q.link.size();
  if (n < 2 || Q.link.empty()) return 0;
  if (mode == 1) { memcpy(Q.G.Rwg, I3, 72); Q.G.s = 1.0; } else { memcpy(Q.G.Rwg, g16, 72); Q.G.s = g16[9]; }
  memcpy(Q.G.bg, g16 + 10, 24); memcpy(Q.G.ba, g16 + 13, 24);
  Q.v.resize(3 * n);
  for (int k = 0; k < n; ++k) for (int r = 0; r < 3; ++r) Q.v[3 * k + r] = kfState[21 * k + 12 + r];
  Q.Info.assign((size_t)n * 81, 0.0);
  for (int k : Q.link) Information(Q.P[k], &Q.Info[(size_t)k * 81]);
  int m = Q.freeV ? 3 * n : 0;
  for (int c = 0; c < 9; ++c) { const bool fr = c < 6 ? Q.freeB : (c < 8 ? Q.freeG : Q.freeS); Q.ig[c] = fr ? m++ : -1; }
  Q.m = m;

  std::vector<double> H, b, x(m, 0.0), A;
  int its = 0, trials = 0, ok = 1;
  chi2[0] = Q.Chi2();
  if (Q.lm) {
    double lambda = 0, ni = 2, currentChi = chi2[0];
    int nBad = 0;
    for (int iter = 0; iter < 200; ++iter) {
      ++its;
      currentChi = Q.Chi2();
      const double iniChi = currentChi;
      Q.Build(H, b);
      if (iter == 0) {
        if (mode == 1 || Q.priorG != 0.0) lambda = 1e3;
        else { double mx = 0; for (int i = 0; i < m; ++i) mx = std::max(mx, std::fabs(H[(size_t)i * m + i])); lambda = 1e-5 * mx; }
        ni = 2; nBad = 0;
      }
      double rho = 0;
      int qmax = 0;
      do {
        const std::vector<double> vbk = Q.v;
        const Globals Gbk = Q.G;
        A = H;
        for (int i = 0; i < m; ++i) A[(size_t)i * m + i] += lambda;
        const bool ok2 = SolveDense(m, A, b, x);
        if (!ok2) std::fill(x.begin(), x.end(), 0.0);
        Q.Update(x);
        double tempChi = Q.Chi2();
        if (!ok2) tempChi = std::numeric_limits<double>::max();
        rho = currentChi - tempChi;
        double scale = 0;
        for (int i = 0; i < m; ++i) scale += x[i] * (lambda * x[i] + b[i]);
        scale += 1e-3;
        rho /= scale;
        if (rho > 0 && std::isfinite(tempChi)) {
          double alpha = 1. - std::pow(2 * rho - 1, 3);
          alpha = std::min(alpha, 2. / 3.);
          lambda *= std::max(1. / 3., alpha);
          ni = 2;
          currentChi = tempChi;
        } else {
          lambda *= ni; ni *= 2;
          Q.v = vbk; Q.G = Gbk;
        }
        ++qmax; ++trials;
      } while (rho < 0 && qmax < 10);
      if (qmax == 10 || rho == 0 || !(rho == rho)) break;
      if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
      if (nBad >= 3) break;
    }
    chi2[1] = currentChi;
  } else {
    for (int iter = 0; iter < 10; ++iter) {
      ++its;
      Q.Build(H, b);
      const bool ok2 = SolveDense(m, H, b, x);
      if (!ok2) std::fill(x.begin(), x.end(), 0.0);
      Q.Update(x);
      if (!ok2) { ok = 0; break; }
    }
    chi2[1] = Q.Chi2();
  }
  if (Q.lm) {
    const float bgf[3] = {(float)Q.G.bg[0], (float)Q.G.bg[1], (float)Q.G.bg[2]}, baf[3] = {(float)Q.G.ba[0], (float)Q.G.ba[1], (float)Q.G.ba[2]};
    for (int k = 0; k < n; ++k) {
      float* s = kfState + 21 * k;
      const float d0 = s[15] - bgf[0], d1 = s[16] - bgf[1], d2 = s[17] - bgf[2];
      const float nrm = std::sqrt(d0 * d0 + d1 * d1 + d2 * d2);
      reint[k] = (nrm > 0.01 && k >= 1 && hasLink[k]) ? 1 : 0;
      for (int r = 0; r < 3; ++r) { s[12 + r] = (float)Q.v[3 * k + r]; s[15 + r] = bgf[r]; s[18 + r] = baf[r]; }
    }
  }
  if (mode != 1) { memcpy(g16, Q.G.Rwg, 72); g16[9] = Q.G.s; }
  if (mode != 2) { memcpy(g16 + 10, Q.G.bg, 24); memcpy(g16 + 13, Q.G.ba, 24); }
  stats4[0] = its; stats4[1] = trials; stats4[2] = ok;
  return 1;
}

}  // extern "C"
