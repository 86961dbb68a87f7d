// CPU oracle of the whole-map bundle adjustment of loop closing, Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF,
// bRobust) (reference src/Optimizer.cc:56-362), for the tests: an FP64 restatement written from the reference's behaviour — EdgeSE3ProjectXYZ,
// EdgeStereoSE3ProjectXYZ and EdgeSE3ProjectXYZToBody with their float leaks, the Huber kernels as :171-175, :204-208 and :244-246 set them,
// g2o's Levenberg-Marquardt with ORB-SLAM's stop rule over the Schur complement of the points, computeLambdaInit over the pose and the point
// diagonals.  Poses are rotation matrices (Rodrigues' formula), not quaternions; a vertex without an edge is REMOVED from the system (index
// maps); the reduced camera system is assembled point by point into a skyline (the envelope of its rows) and factorised there by a scalar
// LDL^T, so that a map of a few hundred keyframes stays affordable on one thread.  On a pinhole problem every operation on a value is the one
// tests/native/merge_ba_oracle.cc applies to it, in its order; the zeros outside the envelope are the only ones skipped.  It shares no code
// with the kernels.  Built by tests/global_ba_oracle.py (g++ -O2 -ffp-contract=off; a second way, -O3 -ffp-contract=fast with
// GB_ORACLE_REVERSE: the points are then visited in reverse order).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

namespace {

struct Kb8 { float p[8]; };   // fx fy cx cy k0..k3
struct Cams {
  int kb8;
  float pin[5];               // pinhole: fx fy cx cy bf
  Kb8 L, R;
  double Rrl[9], trl[3];      // mTrl
};

struct Pose { double R[9], t[3]; };

void map_point(const Pose& T, const double* X, double* xc) {
  for (int r = 0; r < 3; ++r) xc[r] = T.R[r * 3] * X[0] + T.R[r * 3 + 1] * X[1] + T.R[r * 3 + 2] * X[2] + T.t[r];
}

// KannalaBrandt8::project(Vector3d): atan2f and sqrtf on doubles, as the reference has them
void kb8_project(const Kb8& c, const double* v, double* uv) {
  const double x2_plus_y2 = v[0] * v[0] + v[1] * v[1];
  const double theta = atan2f(sqrtf((float)x2_plus_y2), (float)v[2]);
  const double psi = atan2f((float)v[1], (float)v[0]);
  const double theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta3 * theta2, theta7 = theta5 * theta2, theta9 = theta7 * theta2;
  const double r = theta + c.p[4] * theta3 + c.p[5] * theta5 + c.p[6] * theta7 + c.p[7] * theta9;
  uv[0] = c.p[0] * r * cos(psi) + c.p[2];
  uv[1] = c.p[1] * r * sin(psi) + c.p[3];
}
void kb8_project_jac(const Kb8& c, const double* v, double* J) {   // KannalaBrandt8::projectJac
  const double x2 = v[0] * v[0], y2 = v[1] * v[1], z2 = v[2] * v[2];
  const double r2 = x2 + y2, r = sqrt(r2), r3 = r2 * r;
  const double theta = atan2(r, v[2]);
  const double t2 = theta * theta, t3 = t2 * theta, t4 = t2 * t2, t5 = t4 * theta, t6 = t2 * t4, t7 = t6 * theta, t8 = t4 * t4, t9 = t8 * theta;
  const double f = theta + t3 * c.p[4] + t5 * c.p[5] + t7 * c.p[6] + t9 * c.p[7];
  const double fd = 1 + 3 * c.p[4] * t2 + 5 * c.p[5] * t4 + 7 * c.p[6] * t6 + 9 * c.p[7] * t8;
  J[0] = c.p[0] * (fd * v[2] * x2 / (r2 * (r2 + z2)) + f * y2 / r3);
  J[3] = c.p[1] * (fd * v[2] * v[1] * v[0] / (r2 * (r2 + z2)) - f * v[1] * v[0] / r3);
  J[1] = c.p[0] * (fd * v[2] * v[1] * v[0] / (r2 * (r2 + z2)) - f * v[1] * v[0] / r3);
  J[4] = c.p[1] * (fd * v[2] * y2 / (r2 * (r2 + z2)) + f * x2 / r3);
  J[2] = -c.p[0] * fd * v[0] / (r2 + z2);
  J[5] = -c.p[1] * fd * v[1] / (r2 + z2);
}

// the kind of an edge: 0 EdgeSE3ProjectXYZ on the pinhole camera, 1 EdgeStereoSE3ProjectXYZ, 2 EdgeSE3ProjectXYZ on the left KannalaBrandt8
// camera, 3 EdgeSE3ProjectXYZToBody (the right one behind mTrl)
int edge_error(const Cams& c, int kind, const double* xc, const float* obs, double* err) {
  if (kind >= 2) {
    double uv[2], xr[3];
    if (kind == 3) {
      for (int r = 0; r < 3; ++r) xr[r] = c.Rrl[r * 3] * xc[0] + c.Rrl[r * 3 + 1] * xc[1] + c.Rrl[r * 3 + 2] * xc[2] + c.trl[r];
      kb8_project(c.R, xr, uv);
    } else kb8_project(c.L, xc, uv);
    err[0] = (double)obs[0] - uv[0]; err[1] = (double)obs[1] - uv[1];
    return 2;
  }
  if (kind == 0) {   // Pinhole::project(Vector3d)
    err[0] = (double)obs[0] - ((double)c.pin[0] * xc[0] / xc[2] + (double)c.pin[2]);
    err[1] = (double)obs[1] - ((double)c.pin[1] * xc[1] / xc[2] + (double)c.pin[3]);
    return 2;
  }
  const float invz = (float)(1.0 / xc[2]);
  const double u = xc[0] * invz * (double)c.pin[0] + (double)c.pin[2];
  const double v = xc[1] * invz * (double)c.pin[1] + (double)c.pin[3];
  err[0] = (double)obs[0] - u; err[1] = (double)obs[1] - v; err[2] = (double)obs[2] - (u - (double)c.pin[4] * invz);
  return 3;
}

// d(projection) / d(xc), rows x 3
void projection_jac(const Cams& c, int kind, const double* v, double* J) {
  if (kind == 2) { kb8_project_jac(c.L, v, J); return; }
  if (kind == 3) {   // projectJac(mTrl.map(xc)) * Rrl
    double xr[3], pj[6];
    for (int r = 0; r < 3; ++r) xr[r] = c.Rrl[r * 3] * v[0] + c.Rrl[r * 3 + 1] * v[1] + c.Rrl[r * 3 + 2] * v[2] + c.trl[r];
    kb8_project_jac(c.R, xr, pj);
    for (int r = 0; r < 2; ++r)
      for (int k = 0; k < 3; ++k) J[r * 3 + k] = pj[r * 3] * c.Rrl[k] + pj[r * 3 + 1] * c.Rrl[3 + k] + pj[r * 3 + 2] * c.Rrl[6 + k];
    return;
  }
  const double fx = c.pin[0], fy = c.pin[1], bf = c.pin[4], z = v[2], z2 = z * z;
  J[0] = fx / z; J[1] = 0; J[2] = -fx * v[0] / z2;
  J[3] = 0; J[4] = fy / z; J[5] = -fy * v[1] / z2;
  if (kind == 1) { J[6] = fx / z; J[7] = 0; J[8] = -fx * v[0] / z2 + bf / z2; }
}

// error (rows), Jacobian by the pose update (rows x 6: rotation, translation; SE3Quat::exp order) and by the point (rows x 3)
int edge(const Cams& c, int kind, const Pose& T, const double* X, const float* obs, double* err, double* Jp, double* Jl) {
  double xc[3], pj[9];
  map_point(T, X, xc);
  const int rows = edge_error(c, kind, xc, obs, err);
  if (!Jp && !Jl) return rows;
  projection_jac(c, kind, xc, pj);
  if (Jl)
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < 3; ++k) Jl[r * 3 + k] = -(pj[r * 3] * T.R[k] + pj[r * 3 + 1] * T.R[3 + k] + pj[r * 3 + 2] * T.R[6 + k]);
  if (Jp) {
    const double S[18] = {0, xc[2], -xc[1], 1, 0, 0, -xc[2], 0, xc[0], 0, 1, 0, xc[1], -xc[0], 0, 0, 0, 1};   // [ -[xc]x | I ]
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < 6; ++k) Jp[r * 6 + k] = -(pj[r * 3] * S[k] + pj[r * 3 + 1] * S[6 + k] + pj[r * 3 + 2] * S[12 + k]);
  }
  return rows;
}

// g2o::SE3Quat::exp(update) * T with rotation matrices
Pose oplus(const Pose& T, const double* u) {
  const double w[3] = {u[0], u[1], u[2]}, theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double Om[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double Om2[9], R[9], V[9];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Om2[i * 3 + j] = Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j] + Om[i * 3 + 2] * Om[6 + j];
  double a = 1, b = 1, cc = 1;   // theta < 1e-5: R = I + Omega + Omega^2, V = R (se3quat.h)
  if (!(theta < 0.00001)) { a = sin(theta) / theta; b = (1 - cos(theta)) / (theta * theta); cc = (theta - sin(theta)) / pow(theta, 3); }
  for (int i = 0; i < 9; ++i) {
    const double id = (i % 4 == 0) ? 1.0 : 0.0;
    R[i] = id + a * Om[i] + b * Om2[i];
    V[i] = theta < 0.00001 ? R[i] : id + b * Om[i] + cc * Om2[i];
  }
  double te[3];
  for (int i = 0; i < 3; ++i) te[i] = V[i * 3] * u[3] + V[i * 3 + 1] * u[4] + V[i * 3 + 2] * u[5];
  Pose o;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o.R[i * 3 + j] = R[i * 3] * T.R[j] + R[i * 3 + 1] * T.R[3 + j] + R[i * 3 + 2] * T.R[6 + j];
    o.t[i] = R[i * 3] * T.t[0] + R[i * 3 + 1] * T.t[1] + R[i * 3 + 2] * T.t[2] + te[i];
  }
  return o;
}

double huber_rho(double delta, double e, double* w) {   // RobustKernelHuber::robustify
  const double dsqr = delta * delta;
  if (e <= dsqr) { *w = 1; return e; }
  const double sqrte = sqrt(e);
  *w = delta / sqrte;
  return 2 * sqrte * delta - dsqr;
}

void inv3(const double* m, double* o) {
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double id = 1.0 / (m[0] * c00 + m[1] * c01 + m[2] * c02);
  o[0] = c00 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  o[3] = c01 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  o[6] = c02 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

// The lower triangle of a symmetric m x m matrix, row r kept from column first[r] on (its envelope): (r, c) is at off[r] + c - first[r].
struct Skyline {
  int m = 0;
  std::vector<int> first;
  std::vector<size_t> off;
  std::vector<double> a;
  double& at(int r, int c) { return a[off[r] + (size_t)(c - first[r])]; }
  bool has(int r, int c) const { return c >= first[r]; }
};

// LDL^T inside the envelope and the solve (A destroyed): false on a zero or NaN pivot.  Every entry receives what a right-looking dense
// LDL^T gives it — A(i, k) -= A(i, j) A(k, j) / d_j for j ascending, column j divided by d_j behind its last use — without the zeros.
bool skyline_solve(Skyline& A, std::vector<double>& x) {
  const int m = A.m;
  std::vector<double> d(m);
  for (int i = 0; i < m; ++i) {
    // row i, columns k ascending; every entry stays unscaled until the factorisation is done
    for (int k = A.first[i]; k <= i; ++k) {
      double v = A.at(i, k);
      for (int j = std::max(A.first[i], A.first[k]); j < k; ++j) v -= A.at(i, j) * A.at(k, j) / d[j];
      A.at(i, k) = v;
    }
    d[i] = A.at(i, i);
    if (d[i] == 0 || d[i] != d[i]) return false;
  }
  for (int i = 0; i < m; ++i) for (int k = A.first[i]; k < i; ++k) A.at(i, k) /= d[k];
  for (int i = 0; i < m; ++i) for (int j = A.first[i]; j < i; ++j) x[i] -= A.at(i, j) * x[j];
  for (int i = 0; i < m; ++i) x[i] /= d[i];
  for (int j = m - 1; j >= 0; --j) for (int i = A.first[j]; i < j; ++i) x[i] -= A.at(j, i) * x[j];
  return true;
}

Pose pose_from_float7(const float* p) {   // g2o::SE3Quat(q.cast<double>(), t.cast<double>()): the quaternion is normalised in double
  double q[4] = {p[0], p[1], p[2], p[3]};
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (double& v : q) v /= n;
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                       2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
  Pose T;
  memcpy(T.R, R, sizeof R);
  for (int k = 0; k < 3; ++k) T.t[k] = p[4 + k];
  return T;
}

void pose_to_float7(const Pose& T, float* p) {   // rotation -> unit quaternion with w >= 0 (Eigen's branches), cast to float
  const double* m = T.R;
  double q[4];
  const double tr = m[0] + m[4] + m[8];
  if (tr > 0) {
    double t = std::sqrt(tr + 1.0);
    q[3] = 0.5 * t; t = 0.5 / t;
    q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double t = std::sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0);
    q[i] = 0.5 * t; t = 0.5 / t;
    q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t; q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t; q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
  }
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) * (q[3] < 0 ? -1.0 : 1.0);
  for (int k = 0; k < 4; ++k) p[k] = (float)(q[k] / n);
  for (int k = 0; k < 3; ++k) p[4 + k] = (float)T.t[k];
}

struct Graph {
  Cams cam;
  int nKF, nMP, nE;
  const uint8_t* fixed;
  const int *eKF, *eMP;
  const float *obs, *info;
  std::vector<uint8_t> kind;        // [nE]
  std::vector<Pose> T;
  std::vector<double> X;            // [nMP][3]
  std::vector<std::vector<int>> byPoint;
  bool robust;
  double deltaMono, deltaStereo;

  int point(int k) const {
#ifdef GB_ORACLE_REVERSE
    return nMP - 1 - k;
#else
    return k;
#endif
  }
  // the kernel of an edge: 0 = none.  A ToBody edge carries Huber's whatever bRobust says (:244-246)
  double delta(int e) const {
    if (kind[e] == 3) return deltaMono;
    if (!robust) return 0;
    return kind[e] == 1 ? deltaStereo : deltaMono;
  }
  double edge_chi2(int e) const {
    double r[3];
    const int rows = edge(cam, kind[e], T[eKF[e]], &X[3 * eMP[e]], obs + 3 * e, r, nullptr, nullptr);
    double c = 0;
    for (int k = 0; k < rows; ++k) c += r[k] * ((double)info[e] * r[k]);
    return c;
  }
  // computeActiveErrors + activeRobustChi2
  double active_chi2() {
    double s = 0;
    for (int k = 0; k < nMP; ++k)
      for (int e : byPoint[point(k)]) {
        const double c = edge_chi2(e), dl = delta(e);
        double w;
        s += dl > 0 ? huber_rho(dl, c, &w) : c;
      }
    return s;
  }
};

// optimize(iterations).  stats4 = outer iterations, trials, keyframes in the system, envelope blocks; chi2 = before, after
void optimize(Graph& g, int iterations, const volatile uint8_t* stop, int* stats4, double* chi2) {
  int its = 0, trials = 0;
  std::vector<int> col(g.nKF, -1), row(g.nMP, -1);
  std::vector<char> kfUsed(g.nKF, 0);
  int nL = 0;
  for (int m = 0; m < g.nMP; ++m) {
    for (int e : g.byPoint[m]) kfUsed[g.eKF[e]] = 1;
    if (!g.byPoint[m].empty()) row[m] = nL++;
  }
  int nF = 0;
  for (int i = 0; i < g.nKF; ++i) if (kfUsed[i] && !g.fixed[i]) col[i] = nF++;
  const int P = 6 * nF;
  // the envelope of the block rows: row c reaches back to the first free keyframe it shares a point with
  std::vector<int> firstBlock(nF);
  for (int c = 0; c < nF; ++c) firstBlock[c] = c;
  for (int m = 0; m < g.nMP; ++m) {
    int lo = nF;
    for (int e : g.byPoint[m]) if (col[g.eKF[e]] >= 0) lo = std::min(lo, col[g.eKF[e]]);
    for (int e : g.byPoint[m]) if (col[g.eKF[e]] >= 0) firstBlock[col[g.eKF[e]]] = std::min(firstBlock[col[g.eKF[e]]], lo);
  }
  Skyline S;
  S.m = P; S.first.resize(P); S.off.resize(P + 1);
  size_t total = 0;
  int nBlocks = 0;
  for (int c = 0; c < nF; ++c) nBlocks += c - firstBlock[c] + 1;
  for (int r = 0; r < P; ++r) { S.first[r] = 6 * firstBlock[r / 6]; S.off[r] = total; total += (size_t)(r - S.first[r] + 1); }
  if (P) S.off[P] = total;
  S.a.resize(total);
  stats4[2] = nF; stats4[3] = nBlocks;
  struct EdgeLin { int e, c, rows; double Jp[18], Jl[9], err[3], w; };
  std::vector<std::vector<EdgeLin>> lin(g.nMP);
  std::vector<double> Hpp((size_t)36 * nF), bp(P), Hll((size_t)9 * nL), bl((size_t)3 * nL), Dinv((size_t)9 * nL), r(P), xl((size_t)3 * nL);
  double lambda = 0, ni = 2, currentChi = 0;
  int nBad = 0;
  for (int iter = 0; iter < iterations; ++iter) {
    if (stop && *stop) break;
    ++its;
    currentChi = g.active_chi2();
    if (iter == 0) chi2[0] = currentChi;
    const double iniChi = currentChi;
    // buildSystem
    std::fill(Hpp.begin(), Hpp.end(), 0.0); std::fill(bp.begin(), bp.end(), 0.0);
    std::fill(Hll.begin(), Hll.end(), 0.0); std::fill(bl.begin(), bl.end(), 0.0);
    for (int k = 0; k < g.nMP; ++k) {
      const int m = g.point(k);
      lin[m].clear();
      if (row[m] < 0) continue;
      for (int e : g.byPoint[m]) {
        EdgeLin L;
        L.e = e; L.c = col[g.eKF[e]];
        L.rows = edge(g.cam, g.kind[e], g.T[g.eKF[e]], &g.X[3 * m], g.obs + 3 * e, L.err, L.Jp, L.Jl);
        const double info = g.info[e];
        double c = 0;
        for (int q = 0; q < L.rows; ++q) c += L.err[q] * (info * L.err[q]);
        L.w = 1;
        if (g.delta(e) > 0) huber_rho(g.delta(e), c, &L.w);
        double* H = &Hll[(size_t)9 * row[m]];
        double* b = &bl[(size_t)3 * row[m]];
        for (int a = 0; a < 3; ++a) {
          for (int q = 0; q < L.rows; ++q) b[a] += -(L.Jl[q * 3 + a] * L.err[q]) * info * L.w;
          for (int cc = 0; cc < 3; ++cc)
            for (int q = 0; q < L.rows; ++q) H[a * 3 + cc] += L.Jl[q * 3 + a] * L.Jl[q * 3 + cc] * info * L.w;
        }
        if (L.c >= 0)
          for (int a = 0; a < 6; ++a) {
            for (int q = 0; q < L.rows; ++q) bp[6 * L.c + a] += -(L.Jp[q * 6 + a] * L.err[q]) * info * L.w;
            for (int cc = 0; cc < 6; ++cc)
              for (int q = 0; q < L.rows; ++q) Hpp[(size_t)36 * L.c + a * 6 + cc] += L.Jp[q * 6 + a] * L.Jp[q * 6 + cc] * info * L.w;
          }
        lin[m].push_back(L);
      }
    }
    if (iter == 0) {   // computeLambdaInit: tau * the largest diagonal entry over the poses and the points
      double md = 0;
      for (int k = 0; k < P; ++k) md = std::max(md, std::fabs(Hpp[(size_t)36 * (k / 6) + (k % 6) * 7]));
      for (int k = 0; k < nL; ++k) for (int a = 0; a < 3; ++a) md = std::max(md, std::fabs(Hll[(size_t)9 * k + a * 4]));
      lambda = 1e-5 * md;
      ni = 2; nBad = 0;
    }
    double rho = 0;
    int qmax = 0;
    do {
      const std::vector<Pose> Tbk = g.T;
      const std::vector<double> Xbk = g.X;
      // Schur complement of the points with lambda on every diagonal
      std::fill(S.a.begin(), S.a.end(), 0.0);
      for (int c = 0; c < nF; ++c)
        for (int i = 0; i < 6; ++i)
          for (int j = 0; j <= i; ++j) S.at(6 * c + i, 6 * c + j) = Hpp[(size_t)36 * c + i * 6 + j];
      r = bp;
      for (int k = 0; k < P; ++k) S.at(k, k) += lambda;
      for (int k = 0; k < g.nMP; ++k) {
        const int m = g.point(k);
        if (row[m] < 0) continue;
        double D[9];
        memcpy(D, &Hll[(size_t)9 * row[m]], sizeof D);
        D[0] += lambda; D[4] += lambda; D[8] += lambda;
        double* Di = &Dinv[(size_t)9 * row[m]];
        inv3(D, Di);
        const double* b = &bl[(size_t)3 * row[m]];
        // W_i = Jp_i^T (w info) Jl_i of every edge to a free keyframe
        std::vector<double> W(lin[m].size() * 18), WD(lin[m].size() * 18);
        for (size_t a = 0; a < lin[m].size(); ++a) {
          const EdgeLin& L = lin[m][a];
          if (L.c < 0) continue;
          const double wi = g.info[L.e] * L.w;
          for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 3; ++j) {
              double s = 0;
              for (int q = 0; q < L.rows; ++q) s += L.Jp[q * 6 + i] * wi * L.Jl[q * 3 + j];
              W[a * 18 + i * 3 + j] = s;
            }
          for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 3; ++j) WD[a * 18 + i * 3 + j] = W[a * 18 + i * 3] * Di[j] + W[a * 18 + i * 3 + 1] * Di[3 + j] + W[a * 18 + i * 3 + 2] * Di[6 + j];
        }
        for (size_t a = 0; a < lin[m].size(); ++a) {
          const int ca = lin[m][a].c;
          if (ca < 0) continue;
          for (int i = 0; i < 6; ++i) r[6 * ca + i] -= WD[a * 18 + i * 3] * b[0] + WD[a * 18 + i * 3 + 1] * b[1] + WD[a * 18 + i * 3 + 2] * b[2];
          for (size_t b2 = 0; b2 < lin[m].size(); ++b2) {
            const int cb = lin[m][b2].c;
            if (cb < 0 || cb > ca) continue;   // (the lower triangle)
            for (int i = 0; i < 6; ++i)
              for (int j = 0; j < (ca == cb ? i + 1 : 6); ++j)
                S.at(6 * ca + i, 6 * cb + j) -= WD[a * 18 + i * 3] * W[b2 * 18 + j * 3] + WD[a * 18 + i * 3 + 1] * W[b2 * 18 + j * 3 + 1] + WD[a * 18 + i * 3 + 2] * W[b2 * 18 + j * 3 + 2];
          }
        }
      }
      std::vector<double> xp = r;
      const bool ok2 = P == 0 ? true : skyline_solve(S, xp);
      std::fill(xl.begin(), xl.end(), 0.0);
      if (!ok2) std::fill(xp.begin(), xp.end(), 0.0);
      else
        for (int m = 0; m < g.nMP; ++m) {
          if (row[m] < 0) continue;
          double cl[3] = {bl[(size_t)3 * row[m]], bl[(size_t)3 * row[m] + 1], bl[(size_t)3 * row[m] + 2]};
          for (const EdgeLin& L : lin[m]) {
            if (L.c < 0) continue;
            const double wi = g.info[L.e] * L.w;
            for (int j = 0; j < 3; ++j)
              for (int i = 0; i < 6; ++i) {
                double s = 0;
                for (int q = 0; q < L.rows; ++q) s += L.Jp[q * 6 + i] * wi * L.Jl[q * 3 + j];
                cl[j] -= s * xp[6 * L.c + i];
              }
          }
          const double* Di = &Dinv[(size_t)9 * row[m]];
          for (int j = 0; j < 3; ++j) xl[(size_t)3 * row[m] + j] = Di[j * 3] * cl[0] + Di[j * 3 + 1] * cl[1] + Di[j * 3 + 2] * cl[2];
        }
      for (int i = 0; i < g.nKF; ++i) if (col[i] >= 0) g.T[i] = oplus(g.T[i], &xp[6 * col[i]]);
      for (int m = 0; m < g.nMP; ++m) if (row[m] >= 0) for (int j = 0; j < 3; ++j) g.X[3 * m + j] += xl[(size_t)3 * row[m] + j];
      double tempChi = g.active_chi2();
      if (!ok2) tempChi = std::numeric_limits<double>::max();
      double scale = 0;
      for (int k = 0; k < P; ++k) scale += xp[k] * (lambda * xp[k] + bp[k]);
      for (int k = 0; k < 3 * nL; ++k) scale += xl[k] * (lambda * xl[k] + bl[k]);
      scale += 1e-3;
      rho = (currentChi - tempChi) / scale;
      if (rho > 0 && std::isfinite(tempChi)) {
        double alpha = 1. - pow(2 * rho - 1, 3);
        alpha = std::min(alpha, 2. / 3.);
        lambda *= std::max(1. / 3., alpha);
        ni = 2;
        currentChi = tempChi;
      } else {
        lambda *= ni;
        ni *= 2;
        g.T = Tbk; g.X = Xbk;
      }
      ++qmax; ++trials;
    } while (rho < 0 && qmax < 10 && !(stop && *stop));
    if (qmax == 10 || rho == 0) break;
    if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
    if (nBad >= 3) break;
  }
  stats4[0] = its; stats4[1] = trials;
  chi2[1] = currentChi;
}

}  // namespace

extern "C" {

// The flattened problem of morb_bundle_adjustment[_fisheye].  kb8 = 0: eObs3 = (x, y, uRight), cam5 = fx fy cx cy bf.  kb8 != 0: eObs3 = (x, y,
// unused), eRight[e] != 0 marks a ToBody edge, camL8 / camR8 / Trl7 the rig.  Outputs: kfPose of the free keyframes that carry an edge and
// mpPos of the points that carry one, in place; stats4; chi2[2].  No free keyframe with an edge, or stopEntry: nothing written, zeros.
void gb_oracle_run(int kb8, const float* cam5, const float* camL8, const float* camR8, const float* Trl7, int nKF, float* kfPose,
                   const uint8_t* kfFixed, int nMP, float* mpPos, int nE, const int* eKF, const int* eMP, const float* eObs3, const uint8_t* eRight,
                   const float* eInvSigma2, int nIterations, int robust, int stopEntry, int* stats4, double* chi2) {
  memset(stats4, 0, 16); chi2[0] = chi2[1] = 0;
  if (stopEntry) return;
  Graph g;
  memset(&g.cam, 0, sizeof g.cam);
  g.cam.kb8 = kb8;
  if (kb8) {
    memcpy(g.cam.L.p, camL8, 32); memcpy(g.cam.R.p, camR8, 32);
    const Pose Trl = pose_from_float7(Trl7);
    memcpy(g.cam.Rrl, Trl.R, 72); memcpy(g.cam.trl, Trl.t, 24);
  } else memcpy(g.cam.pin, cam5, 20);
  g.nKF = nKF; g.nMP = nMP; g.nE = nE; g.fixed = kfFixed; g.eKF = eKF; g.eMP = eMP; g.info = eInvSigma2; g.obs = eObs3;
  g.kind.resize(nE);
  for (int e = 0; e < nE; ++e) g.kind[e] = kb8 ? (eRight[e] ? 3 : 2) : (eObs3[3 * e + 2] < 0 ? 0 : 1);
  bool any = false;
  for (int e = 0; e < nE; ++e) any = any || !kfFixed[eKF[e]];
  if (!any) return;
  for (int i = 0; i < nKF; ++i) g.T.push_back(pose_from_float7(kfPose + 7 * i));
  g.X.assign(mpPos, mpPos + (size_t)3 * nMP);
  g.byPoint.resize(nMP);
  for (int e = 0; e < nE; ++e) g.byPoint[eMP[e]].push_back(e);
  g.robust = robust != 0;
  g.deltaMono = (double)(float)std::sqrt(5.99); g.deltaStereo = (double)(float)std::sqrt(7.815);   // thHuber2D, thHuber3D (:126-127)
  optimize(g, nIterations, nullptr, stats4, chi2);
  std::vector<char> kfUsed(nKF, 0);
  for (int e = 0; e < nE; ++e) kfUsed[eKF[e]] = 1;
  for (int i = 0; i < nKF; ++i) if (!kfFixed[i] && kfUsed[i]) pose_to_float7(g.T[i], kfPose + 7 * i);
  for (int m = 0; m < nMP; ++m) if (!g.byPoint[m].empty()) for (int k = 0; k < 3; ++k) mpPos[3 * m + k] = (float)g.X[3 * m + k];
}

}  // extern "C"
