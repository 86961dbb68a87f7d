// CPU oracle of the welding bundle adjustment of map merging, Optimizer::LocalBundleAdjustment(KeyFrame* pMainKF, vector<KeyFrame*> vpAdjustKF,
// vector<KeyFrame*> vpFixedKF, bool* pbStopFlag) (reference src/Optimizer.cc:3430-3851), for the tests: an independent FP64 restatement written
// from the reference's behaviour — EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ with their float leaks, Huber kernels, g2o's Levenberg-Marquardt
// with ORB-SLAM's stop rule over the Schur complement of the points, edge levels, the active set of initializeOptimization(level) — with a round
// plan as a parameter (iterations, robust kernel, monocular delta^2 per round).  Poses are rotation matrices (Rodrigues' formula), not
// quaternions; a vertex without an active edge is REMOVED from the system (index maps), not carried along with empty blocks; the reduced
// camera system is assembled point by point.  It shares no code with the kernels.  Built by tests/merge_ba_oracle.py (g++ -O2
// -ffp-contract=off; a second way, -O3 -ffp-contract=fast with MB_ORACLE_REVERSE: the points are then visited in reverse order).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

namespace {

struct Cam { int kb8; float p[8]; };   // pinhole: fx fy cx cy bf; KannalaBrandt8: fx fy cx cy k0..k3

struct Pose { double R[9], t[3]; };

void map_point(const Pose& T, const double* X, double* xc) {
  for (int r = 0; r < 3; ++r) xc[r] = T.R[r * 3] * X[0] + T.R[r * 3 + 1] * X[1] + T.R[r * 3 + 2] * X[2] + T.t[r];
}

// computeError of one edge: rows = 2 (monocular) or 3 (stereo).  obs[2] >= 0: EdgeStereoSE3ProjectXYZ (`const float invz`, cam_project)
int edge_error(const Cam& c, const double* xc, const float* obs, double* err) {
  if (c.kb8) {   // KannalaBrandt8::project(Vector3d): atan2f and sqrtf on doubles, as the reference has them
    const double x2_plus_y2 = xc[0] * xc[0] + xc[1] * xc[1];
    const double theta = atan2f(sqrtf((float)x2_plus_y2), (float)xc[2]);
    const double psi = atan2f((float)xc[1], (float)xc[0]);
    const double theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta3 * theta2, theta7 = theta5 * theta2, theta9 = theta7 * theta2;
    const double r = theta + c.p[4] * theta3 + c.p[5] * theta5 + c.p[6] * theta7 + c.p[7] * theta9;
    err[0] = (double)obs[0] - (c.p[0] * r * cos(psi) + c.p[2]);
    err[1] = (double)obs[1] - (c.p[1] * r * sin(psi) + c.p[3]);
    return 2;
  }
  if (obs[2] < 0) {   // Pinhole::project(Vector3d)
    err[0] = (double)obs[0] - ((double)c.p[0] * xc[0] / xc[2] + (double)c.p[2]);
    err[1] = (double)obs[1] - ((double)c.p[1] * xc[1] / xc[2] + (double)c.p[3]);
    return 2;
  }
  const float invz = (float)(1.0 / xc[2]);
  const double u = xc[0] * invz * (double)c.p[0] + (double)c.p[2];
  const double v = xc[1] * invz * (double)c.p[1] + (double)c.p[3];
  err[0] = (double)obs[0] - u; err[1] = (double)obs[1] - v; err[2] = (double)obs[2] - (u - (double)c.p[4] * invz);
  return 3;
}

// d(projection) / d(xc), rows x 3
void projection_jac(const Cam& c, bool stereo, const double* v, double* J) {
  if (c.kb8) {   // KannalaBrandt8::projectJac
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
    return;
  }
  const double fx = c.p[0], fy = c.p[1], bf = c.p[4], z = v[2], z2 = z * z;
  J[0] = fx / z; J[1] = 0; J[2] = -fx * v[0] / z2;
  J[3] = 0; J[4] = fy / z; J[5] = -fy * v[1] / z2;
  if (stereo) { J[6] = fx / z; J[7] = 0; J[8] = -fx * v[0] / z2 + bf / z2; }
}

// error (rows), Jacobian by the pose update (rows x 6: rotation, translation; SE3Quat::exp order) and by the point (rows x 3)
int edge(const Cam& c, const Pose& T, const double* X, const float* obs, double* err, double* Jp, double* Jl) {
  double xc[3], pj[9];
  map_point(T, X, xc);
  const int rows = edge_error(c, xc, obs, err);
  if (!Jp && !Jl) return rows;
  projection_jac(c, rows == 3, xc, pj);
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

// dense LDL^T of the m x m system (row-major, destroyed): false on a zero or NaN pivot
bool ldlt_solve(std::vector<double>& A, std::vector<double>& x, int m) {
  for (int j = 0; j < m; ++j) {
    const double d = A[(size_t)j * m + j];
    if (d == 0 || d != d) return false;
    for (int i = j + 1; i < m; ++i)
      for (int k = j + 1; k <= i; ++k) A[(size_t)i * m + k] -= A[(size_t)i * m + j] * A[(size_t)k * m + j] / d;
    for (int i = j + 1; i < m; ++i) A[(size_t)i * m + j] /= d;
  }
  for (int j = 0; j < m; ++j) for (int i = j + 1; i < m; ++i) x[i] -= A[(size_t)i * m + j] * x[j];
  for (int i = 0; i < m; ++i) x[i] /= A[(size_t)i * m + i];
  for (int j = m - 1; j >= 0; --j) for (int i = 0; i < j; ++i) x[i] -= A[(size_t)j * m + i] * x[j];
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
  Cam cam;
  int nKF, nMP, nE;
  const uint8_t* fixed;
  const int *eKF, *eMP;
  const float *obs, *info;
  std::vector<Pose> T;
  std::vector<double> X;            // [nMP][3]
  std::vector<uint8_t> level;       // [nE]
  std::vector<double> chi;          // [nE] chi2() of each edge: the last computeActiveErrors that had it active
  std::vector<std::vector<int>> byPoint;
  bool robust;
  double deltaMono, deltaStereo;

  int point(int k) const {
#ifdef MB_ORACLE_REVERSE
    return nMP - 1 - k;
#else
    return k;
#endif
  }
  double edge_chi2(int e, double* err = nullptr) const {
    double r[3];
    const int rows = edge(cam, T[eKF[e]], &X[3 * eMP[e]], obs + 3 * e, r, nullptr, nullptr);
    double c = 0;
    for (int k = 0; k < rows; ++k) c += r[k] * ((double)info[e] * r[k]);
    if (err) memcpy(err, r, sizeof r);
    return c;
  }
  bool depth_positive(int e) const {
    double xc[3];
    map_point(T[eKF[e]], &X[3 * eMP[e]], xc);
    return xc[2] > 0.0;
  }
  // computeActiveErrors + activeRobustChi2
  double active_chi2() {
    double s = 0;
    for (int k = 0; k < nMP; ++k)
      for (int e : byPoint[point(k)]) {
        if (level[e]) continue;
        const double c = chi[e] = edge_chi2(e);
        double w;
        s += robust ? huber_rho(obs[3 * e + 2] < 0 || cam.kb8 ? deltaMono : deltaStereo, c, &w) : c;
      }
    return s;
  }
};

// optimize(iterations) on the active edges (level 0).  Returns (outer iterations, trials); *rejectedLast = the last trial was rejected.
void optimize(Graph& g, int iterations, double userLambda, const volatile uint8_t* stop, int* its, int* trials, int* rejectedLast) {
  *its = *trials = *rejectedLast = 0;
  // initializeOptimization(level): the vertices that have an active edge
  std::vector<int> col(g.nKF, -1), row(g.nMP, -1);
  std::vector<char> kfUsed(g.nKF, 0);
  int nL = 0;
  for (int m = 0; m < g.nMP; ++m) {
    bool used = false;
    for (int e : g.byPoint[m]) if (!g.level[e]) { used = true; kfUsed[g.eKF[e]] = 1; }
    if (used) row[m] = nL++;
  }
  int nF = 0;
  for (int i = 0; i < g.nKF; ++i) if (kfUsed[i] && !g.fixed[i]) col[i] = nF++;
  const int P = 6 * nF;
  struct EdgeLin { int e, c, rows; double Jp[18], Jl[9], err[3], w; };
  std::vector<std::vector<EdgeLin>> lin(g.nMP);
  std::vector<double> Hpp((size_t)P * P), bp(P), Hll((size_t)9 * nL), bl((size_t)3 * nL), Dinv((size_t)9 * nL), S((size_t)P * P), r(P), xl((size_t)3 * nL);
  double lambda = 0, ni = 2;
  int nBad = 0;
  for (int iter = 0; iter < iterations; ++iter) {
    if (stop && *stop) break;
    ++*its;
    double currentChi = g.active_chi2();
    const double iniChi = currentChi;
    // buildSystem
    std::fill(Hpp.begin(), Hpp.end(), 0.0); std::fill(bp.begin(), bp.end(), 0.0);
    std::fill(Hll.begin(), Hll.end(), 0.0); std::fill(bl.begin(), bl.end(), 0.0);
    for (int k = 0; k < g.nMP; ++k) {
      const int m = g.point(k);
      lin[m].clear();
      if (row[m] < 0) continue;
      for (int e : g.byPoint[m]) {
        if (g.level[e]) continue;
        EdgeLin L;
        L.e = e; L.c = col[g.eKF[e]];
        L.rows = edge(g.cam, g.T[g.eKF[e]], &g.X[3 * m], g.obs + 3 * e, L.err, L.Jp, L.Jl);
        const double info = g.info[e];
        double c = 0;
        for (int q = 0; q < L.rows; ++q) c += L.err[q] * (info * L.err[q]);
        L.w = 1;
        if (g.robust) huber_rho(L.rows == 2 ? g.deltaMono : g.deltaStereo, c, &L.w);
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
              for (int q = 0; q < L.rows; ++q) Hpp[(size_t)(6 * L.c + a) * P + 6 * L.c + cc] += L.Jp[q * 6 + a] * L.Jp[q * 6 + cc] * info * L.w;
          }
        lin[m].push_back(L);
      }
    }
    if (iter == 0) {   // computeLambdaInit
      double md = 0;
      for (int k = 0; k < P; ++k) md = std::max(md, std::fabs(Hpp[(size_t)k * P + k]));
      for (int k = 0; k < nL; ++k) for (int a = 0; a < 3; ++a) md = std::max(md, std::fabs(Hll[(size_t)9 * k + a * 4]));
      lambda = userLambda > 0 ? userLambda : 1e-5 * md;
      ni = 2; nBad = 0;
    }
    double rho = 0;
    int qmax = 0;
    do {
      const std::vector<Pose> Tbk = g.T;
      const std::vector<double> Xbk = g.X;
      // Schur complement of the points with lambda on every diagonal
      S = Hpp; r = bp;
      for (int k = 0; k < P; ++k) S[(size_t)k * P + k] += lambda;
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
            if (cb < 0) continue;
            for (int i = 0; i < 6; ++i)
              for (int j = 0; j < 6; ++j)
                S[(size_t)(6 * ca + i) * P + 6 * cb + j] -= WD[a * 18 + i * 3] * W[b2 * 18 + j * 3] + WD[a * 18 + i * 3 + 1] * W[b2 * 18 + j * 3 + 1] + WD[a * 18 + i * 3 + 2] * W[b2 * 18 + j * 3 + 2];
          }
        }
      }
      std::vector<double> xp = r;
      const bool ok2 = P == 0 ? true : ldlt_solve(S, xp, P);
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
        *rejectedLast = 0;
      } else {
        lambda *= ni;
        ni *= 2;
        g.T = Tbk; g.X = Xbk;
        *rejectedLast = 1;
      }
      ++qmax; ++*trials;
    } while (rho < 0 && qmax < 10 && !(stop && *stop));
    if (qmax == 10 || rho == 0) break;
    if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
    if (nBad >= 3) break;
  }
}

}  // namespace

extern "C" {

// error (3; the third row 0 for a monocular edge), Jp (3 x 6), Jl (3 x 3) of one edge; T12 = R (9, row-major) then t, in double; obs3[2] < 0: monocular.
// Returns the rows of the edge.
int mb_oracle_edge(int kb8, const float* cam8, const double* T12, const double* X, const float* obs3, double* err, double* Jp, double* Jl) {
  Cam c; c.kb8 = kb8; memcpy(c.p, cam8, 32);
  Pose T; memcpy(T.R, T12, 72); memcpy(T.t, T12 + 9, 24);
  memset(err, 0, 24); memset(Jp, 0, 144); memset(Jl, 0, 72);
  return edge(c, T, X, obs3, err, Jp, Jl);
}
void mb_oracle_oplus(const double* T12, const double* u, double* out12) {
  Pose T; memcpy(T.R, T12, 72); memcpy(T.t, T12 + 9, 24);
  const Pose o = oplus(T, u);
  memcpy(out12, o.R, 72); memcpy(out12 + 9, o.t, 24);
}

// The flattened problem of morb_merge_bundle_adjustment (eObs = [nE][3]; kb8: every edge monocular on the KannalaBrandt8 camera cam8, the third
// slot ignored).  Round plan: nRounds rounds of planIters[r] iterations, planRobust[r], monocular delta^2 planDelta2[r] (the stereo delta^2 is
// 7.815); between two rounds every edge with chi2() > 5.991 / 7.815 or a non-positive depth goes to level 1.  stopEntry: *pbStopFlag at entry;
// stopAfter: raised when that many rounds have run (0 = never).  Outputs: kfPose / mpPos in place (free keyframes that carry an edge, all
// points), erase / level [nE], stats6 as the entry's, chiStale / chiFresh [nE] (chi2() as the erase rule reads it; chi2 at the final
// estimate), info4 = {round 1 ended on a rejected trial, points without an active edge in round 2, free keyframes with edges but none
// active in round 2, edges erased on their stale chi2 whose fresh chi2 passes}.
void mb_oracle_run(int kb8, const float* cam8, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos, int nE, const int* eKF,
                   const int* eMP, const float* eObs, const float* eInvSigma2, int nRounds, const int* planIters, const int* planRobust,
                   const double* planDelta2, double userLambda, int stopEntry, int stopAfter, uint8_t* erase, uint8_t* level, int* stats6,
                   double* chiStale, double* chiFresh, int* info4) {
  memset(erase, 0, nE); memset(level, 0, nE); memset(stats6, 0, 24); memset(info4, 0, 16);
  for (int e = 0; e < nE; ++e) chiStale[e] = chiFresh[e] = 0;
  if (stopEntry) return;
  Graph g;
  g.cam.kb8 = kb8; memcpy(g.cam.p, cam8, 32);
  g.nKF = nKF; g.nMP = nMP; g.nE = nE; g.fixed = kfFixed; g.eKF = eKF; g.eMP = eMP; g.info = eInvSigma2;
  std::vector<float> obs(eObs, eObs + (size_t)3 * nE);
  if (kb8) for (int e = 0; e < nE; ++e) obs[3 * e + 2] = -1.f;
  g.obs = obs.data();
  for (int i = 0; i < nKF; ++i) g.T.push_back(pose_from_float7(kfPose + 7 * i));
  g.X.assign(mpPos, mpPos + (size_t)3 * nMP);
  g.level.assign(nE, 0); g.chi.assign(nE, 0.0);
  g.byPoint.resize(nMP);
  for (int e = 0; e < nE; ++e) g.byPoint[eMP[e]].push_back(e);
  volatile uint8_t stop = 0;
  int rounds = 0;
  for (int r = 0; r < nRounds; ++r) {
    if (r > 0) {
      if (stop) break;
      int n1 = 0;
      for (int e = 0; e < nE; ++e) {
        const bool st = !(obs[3 * e + 2] < 0);
        if (g.chi[e] > (st ? 7.815 : 5.991) || !g.depth_positive(e)) { g.level[e] = 1; ++n1; }
      }
      stats6[4] = n1;
      std::vector<char> kfHas(nKF, 0), kfActive(nKF, 0);
      for (int m = 0; m < nMP; ++m) {
        bool any = false;
        for (int e : g.byPoint[m]) { kfHas[eKF[e]] = 1; if (!g.level[e]) { any = true; kfActive[eKF[e]] = 1; } }
        if (!any && !g.byPoint[m].empty()) ++info4[1];
      }
      for (int i = 0; i < nKF; ++i) if (!kfFixed[i] && kfHas[i] && !kfActive[i]) ++info4[2];
    }
    g.robust = planRobust[r] != 0;
    g.deltaMono = (double)(float)std::sqrt(planDelta2[r]); g.deltaStereo = (double)(float)std::sqrt(7.815);
    int its, trials, rej;
    optimize(g, planIters[r], userLambda, &stop, &its, &trials, &rej);
    if (r < 2) { stats6[2 * r] = its; stats6[2 * r + 1] = trials; }
    if (r == 0) info4[0] = rej;
    ++rounds;
    if (stopAfter && rounds >= stopAfter) stop = 1;
  }
  stats6[5] = rounds;
  std::vector<char> kfUsed(nKF, 0);
  for (int e = 0; e < nE; ++e) {
    kfUsed[eKF[e]] = 1;
    const bool st = !(obs[3 * e + 2] < 0);
    const double thr = st ? 7.815 : 5.991;
    chiStale[e] = g.chi[e];
    chiFresh[e] = g.edge_chi2(e);
    level[e] = g.level[e];
    const bool deep = g.depth_positive(e);
    erase[e] = (g.chi[e] > thr || !deep) ? 1 : 0;
    if (g.chi[e] > thr && deep && !(chiFresh[e] > thr)) ++info4[3];
  }
  for (int i = 0; i < nKF; ++i) if (!kfFixed[i] && kfUsed[i]) pose_to_float7(g.T[i], kfPose + 7 * i);
  for (size_t k = 0; k < (size_t)3 * nMP; ++k) mpPos[k] = (float)g.X[k];
}

}  // extern "C"
