// CPU oracle of the numeric part of Tracking::CreateInitialMapMonocular (reference src/Tracking.cc:2345-2430) for the tests: an independent
// restatement written from the reference's behaviour — BundleAdjustment's graph of two keyframes (src/Optimizer.cc:56-362),
// EdgeSE3ProjectXYZ (src/OptimizableTypes.cpp:134-156), g2o's Levenberg-Marquardt with ORB-SLAM's stop rule over the Schur complement of
// the points, ComputeSceneMedianDepth, the rescaling and UpdateNormalAndDepth.  The general sparse formulation: the normal equations are
// assembled DENSE over all 6 + 3 n unknowns from the edges' Jacobians, and the solver then reads its blocks out of that matrix in g2o's
// Schur order.  Poses are rotation matrices (Rodrigues' formula), not quaternions.  It shares no code with the kernel or with
// include/morb/initial_map_math.h.  Built by tests/initial_map_oracle.py (g++ -O2 -ffp-contract=off; a second way, -O3
// -ffp-contract=fast with IM_ORACLE_REVERSE, for the corpus-selection test: the points are then visited in reverse order).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

namespace {

struct Cam { int kb8; float p[8]; };

void project(const Cam& c, const double* v, double* uv) {
  if (!c.kb8) {   // Pinhole::project(Vector3d)
    uv[0] = (double)c.p[0] * v[0] / v[2] + (double)c.p[2];
    uv[1] = (double)c.p[1] * v[1] / v[2] + (double)c.p[3];
    return;
  }
  // KannalaBrandt8::project(Vector3d): atan2f and sqrtf on doubles, as the reference has them
  const double x2_plus_y2 = v[0] * v[0] + v[1] * v[1];
  const double theta = atan2f(sqrtf((float)x2_plus_y2), (float)v[2]);
  const double psi = atan2f((float)v[1], (float)v[0]);
  const double theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta3 * theta2, theta7 = theta5 * theta2, theta9 = theta7 * theta2;
  const double r = theta + c.p[4] * theta3 + c.p[5] * theta5 + c.p[6] * theta7 + c.p[7] * theta9;
  uv[0] = c.p[0] * r * cos(psi) + c.p[2];
  uv[1] = c.p[1] * r * sin(psi) + c.p[3];
}

void project_jac(const Cam& c, const double* v, double* J /* 2 x 3 */) {
  if (!c.kb8) {   // Pinhole::projectJac
    J[0] = c.p[0] / v[2]; J[1] = 0; J[2] = -c.p[0] * v[0] / (v[2] * v[2]);
    J[3] = 0; J[4] = c.p[1] / v[2]; J[5] = -c.p[1] * v[1] / (v[2] * v[2]);
    return;
  }
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

struct Pose { double R[9], t[3]; };

void map_point(const Pose& T, const double* X, double* xc) {
  for (int r = 0; r < 3; ++r) xc[r] = T.R[r * 3] * X[0] + T.R[r * 3 + 1] * X[1] + T.R[r * 3 + 2] * X[2] + T.t[r];
}

// one EdgeSE3ProjectXYZ: error (2), Jacobian by the pose update (2 x 6: rotation, translation; SE3Quat::exp order) and by the point (2 x 3)
void edge(const Cam& c, const Pose& T, const double* X, const double* obs, double* err, double* Jp, double* Jl) {
  double xc[3], uv[2], pj[6];
  map_point(T, X, xc);
  project(c, xc, uv);
  err[0] = obs[0] - uv[0];
  err[1] = obs[1] - uv[1];
  if (!Jp && !Jl) return;
  project_jac(c, xc, pj);
  if (Jl)
    for (int r = 0; r < 2; ++r)
      for (int k = 0; k < 3; ++k) Jl[r * 3 + k] = -(pj[r * 3] * T.R[k] + pj[r * 3 + 1] * T.R[3 + k] + pj[r * 3 + 2] * T.R[6 + k]);
  if (Jp) {
    // SE3deriv = [ -[xc]x | I ]
    const double S[18] = {0, xc[2], -xc[1], 1, 0, 0, -xc[2], 0, xc[0], 0, 1, 0, xc[1], -xc[0], 0, 0, 0, 1};
    for (int r = 0; r < 2; ++r)
      for (int k = 0; k < 6; ++k) Jp[r * 6 + k] = -(pj[r * 3] * S[k] + pj[r * 3 + 1] * S[6 + k] + pj[r * 3 + 2] * S[12 + k]);
  }
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

bool inv3(const double* m, double* o) {
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
  const double id = 1.0 / det;
  o[0] = c00 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  o[3] = c01 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  o[6] = c02 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
  return true;
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

struct Point { double X[3], o1[2], o2[2], w1, w2; int i, j; };

struct Problem {
  Cam cam;
  std::vector<Point> pts;
  Pose T;
  bool robust;
  double delta;

  int order(int k) const {
#ifdef IM_ORACLE_REVERSE
    return (int)pts.size() - 1 - k;
#else
    return k;
#endif
  }
  double chi2() const {
    const Pose I = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
    double s = 0;
    for (int k = 0; k < (int)pts.size(); ++k) {
      const Point& p = pts[order(k)];
      double e[2], w;
      edge(cam, I, p.X, p.o1, e, nullptr, nullptr);
      double c = p.w1 * (e[0] * e[0] + e[1] * e[1]);
      s += robust ? huber_rho(delta, c, &w) : c;
      edge(cam, T, p.X, p.o2, e, nullptr, nullptr);
      c = p.w2 * (e[0] * e[0] + e[1] * e[1]);
      s += robust ? huber_rho(delta, c, &w) : c;
    }
    return s;
  }
  // dense H (N x N) and b (N), N = 6 + 3 n: unknowns = the pose of keyframe 2, then the points
  void build(std::vector<double>& H, std::vector<double>& b) const {
    const int n = (int)pts.size(), N = 6 + 3 * n;
    std::fill(H.begin(), H.end(), 0.0);
    std::fill(b.begin(), b.end(), 0.0);
    const Pose I = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
    for (int k = 0; k < n; ++k) {
      const int q = order(k);
      const Point& p = pts[q];
      for (int kf = 0; kf < 2; ++kf) {
        double e[2], Jp[12], Jl[6], w = 1;
        edge(cam, kf ? T : I, p.X, kf ? p.o2 : p.o1, e, Jp, Jl);
        const double info = kf ? p.w2 : p.w1;
        if (robust) huber_rho(delta, info * (e[0] * e[0] + e[1] * e[1]), &w);
        // the edge's Jacobian row block over the whole unknown vector: columns 0..5 (keyframe 2 only), 6 + 3 q .. 6 + 3 q + 2
        int cols[9]; double J[2][9]; int nc = 0;
        if (kf) for (int c = 0; c < 6; ++c) { cols[nc] = c; J[0][nc] = Jp[c]; J[1][nc] = Jp[6 + c]; ++nc; }
        for (int c = 0; c < 3; ++c) { cols[nc] = 6 + 3 * q + c; J[0][nc] = Jl[c]; J[1][nc] = Jl[3 + c]; ++nc; }
        for (int a = 0; a < nc; ++a) {
          b[cols[a]] += -(J[0][a] * e[0] + J[1][a] * e[1]) * info * w;
          for (int c = 0; c < nc; ++c) H[(size_t)cols[a] * N + cols[c]] += (J[0][a] * J[0][c] + J[1][a] * J[1][c]) * info * w;
        }
      }
    }
  }
};

}  // namespace

extern "C" {

// error (2), Jp (2 x 6), Jl (2 x 3) of one edge; T12 = R (9, row-major) then t, in double
void im_oracle_edge(int kb8, const float* cam8, const double* T12, const double* X, const double* obs, double* err, double* Jp, double* Jl) {
  Cam c; c.kb8 = kb8; memcpy(c.p, cam8, 32);
  Pose T; memcpy(T.R, T12, 72); memcpy(T.t, T12 + 9, 24);
  edge(c, T, X, obs, err, Jp, Jl);
}
// ... and the same pose moved by the update u (for the central differences of the test)
void im_oracle_oplus(const double* T12, const double* u, double* out12) {
  Pose T; memcpy(T.R, T12, 72); memcpy(T.t, T12 + 9, 24);
  const Pose o = oplus(T, u);
  memcpy(out12, o.R, 72); memcpy(out12 + 9, o.t, 24);
}

// One problem.  kp1 / kp2 [n1 / n2][3] = x, y, octave (as floats); matches12, triangulated, P3D by frame-1 keypoint.  Outputs as the entry's rows
// (mpPos, mpNormal [n1][3], mpDist [n1][2], hasMP [n1], stats [4], chi2 [2]).  Returns the status.
int im_oracle_run(int kb8, const float* cam8, const float* levelSigma2, const float* scaleFactors, int nlevels, int n1, const float* kp1, int n2,
                  const float* kp2, const int* matches12, const uint8_t* triangulated, const float* P3D, int ok, const float* T21, int nIterations,
                  int robust, float depthScale, int minTracked, int stop, float* Tcw2, float* mpPos, float* mpNormal, float* mpDist, uint8_t* hasMP,
                  int* stats, double* chi2, float* median) {
  memset(Tcw2, 0, 48); memset(mpPos, 0, 12 * (size_t)n1); memset(mpNormal, 0, 12 * (size_t)n1); memset(mpDist, 0, 8 * (size_t)n1);
  memset(hasMP, 0, (size_t)n1); memset(stats, 0, 16); chi2[0] = chi2[1] = 0; *median = 0;
  if (!ok) return 0;
  Problem pr;
  pr.cam.kb8 = kb8; memcpy(pr.cam.p, cam8, 32);
  pr.robust = robust != 0;
  pr.delta = (double)(float)sqrt(5.99);
  for (int i = 0; i < n1; ++i) {
    const int j = matches12[i];
    if (j < 0 || j >= n2 || !triangulated[i]) continue;
    Point p;
    for (int k = 0; k < 3; ++k) p.X[k] = P3D[3 * i + k];
    p.o1[0] = kp1[3 * i]; p.o1[1] = kp1[3 * i + 1]; p.o2[0] = kp2[3 * j]; p.o2[1] = kp2[3 * j + 1];
    p.w1 = 1.0f / levelSigma2[(int)kp1[3 * i + 2]]; p.w2 = 1.0f / levelSigma2[(int)kp2[3 * j + 2]];
    p.i = i; p.j = j;
    pr.pts.push_back(p);
  }
  {
    // the pose a Sophus::SE3f holds is a float quaternion: g2o::SE3Quat(Tcw.unit_quaternion().cast<double>(), ...) normalises it in double
    // (Optimizer.cc:117-119).  Eigen's matrix -> quaternion in float, then the rotation matrix of the normalised quaternion in double.
    float q[4];
    const float* m = T21;
    float tr = m[0] + m[4] + m[8];
    if (tr > 0) {
      float t = std::sqrt(tr + 1.0f);
      q[3] = 0.5f * t; t = 0.5f / t;
      q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
    } else {
      int i = 0;
      if (m[4] > m[0]) i = 1;
      if (m[8] > m[i * 4]) i = 2;
      const int j = (i + 1) % 3, k = (j + 1) % 3;
      float t = std::sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0f);
      q[i] = 0.5f * t; t = 0.5f / t;
      q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t; q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t; q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
    }
    double d[4] = {q[0], q[1], q[2], q[3]};
    const double nq = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
    for (double& v : d) v /= nq;
    const double x = d[0], y = d[1], z = d[2], w = d[3];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                         2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    memcpy(pr.T.R, R, sizeof R);
  }
  for (int k = 0; k < 3; ++k) pr.T.t[k] = T21[9 + k];
  const int n = (int)pr.pts.size(), N = 6 + 3 * n;
  int its = 0, trials = 0, stopSeen = 0;
  const double chiFirst = pr.chi2();
  double chiLast = chiFirst;
  if (stop) stopSeen = 1;
  else if (n > 0 && nIterations > 0) {
    std::vector<double> H((size_t)N * N), b(N), x(N);
    double lambda = 0, ni = 2, currentChi = chiFirst;
    int nBad = 0;
    for (int iter = 0; iter < nIterations; ++iter) {
      ++its;
      currentChi = pr.chi2();
      const double iniChi = currentChi;
      pr.build(H, b);
      if (iter == 0) {
        double md = 0;
        for (int k = 0; k < N; ++k) md = std::max(md, std::fabs(H[(size_t)k * N + k]));
        lambda = 1e-5 * md;
      }
      double rho = 0;
      int qmax = 0;
      do {
        const Problem backup = pr;
        // g2o's BlockSolver with the points marginalised: Hschur = Hpp + lambda I - sum Hpl (Hll + lambda I)^-1 Hpl^T, read out of the dense H
        std::vector<double> S(36), r(6);
        for (int a = 0; a < 6; ++a) { r[a] = b[a]; for (int c = 0; c < 6; ++c) S[a * 6 + c] = H[(size_t)a * N + c] + (a == c ? lambda : 0.0); }
        std::vector<double> Dinv((size_t)9 * n);
        for (int k = 0; k < n; ++k) {
          const int q = pr.order(k), o = 6 + 3 * q;
          double D[9], W[18], WD[18];
          for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) D[a * 3 + c] = H[(size_t)(o + a) * N + o + c] + (a == c ? lambda : 0.0);
          inv3(D, &Dinv[(size_t)9 * q]);
          const double* Di = &Dinv[(size_t)9 * q];
          for (int a = 0; a < 6; ++a) for (int c = 0; c < 3; ++c) W[a * 3 + c] = H[(size_t)a * N + o + c];
          for (int a = 0; a < 6; ++a) for (int c = 0; c < 3; ++c) WD[a * 3 + c] = W[a * 3] * Di[c] + W[a * 3 + 1] * Di[3 + c] + W[a * 3 + 2] * Di[6 + c];
          for (int a = 0; a < 6; ++a) {
            for (int c = 0; c < 6; ++c) S[a * 6 + c] -= WD[a * 3] * W[c * 3] + WD[a * 3 + 1] * W[c * 3 + 1] + WD[a * 3 + 2] * W[c * 3 + 2];
            r[a] -= WD[a * 3] * b[o] + WD[a * 3 + 1] * b[o + 1] + WD[a * 3 + 2] * b[o + 2];
          }
        }
        const bool ok2 = ldlt_solve(S, r, 6);
        std::fill(x.begin(), x.end(), 0.0);
        if (ok2) {
          for (int a = 0; a < 6; ++a) x[a] = r[a];
          for (int q = 0; q < n; ++q) {
            const int o = 6 + 3 * q;
            double cl[3];
            for (int c = 0; c < 3; ++c) { cl[c] = b[o + c]; for (int a = 0; a < 6; ++a) cl[c] -= H[(size_t)a * N + o + c] * x[a]; }
            const double* Di = &Dinv[(size_t)9 * q];
            for (int c = 0; c < 3; ++c) x[o + c] = Di[c * 3] * cl[0] + Di[c * 3 + 1] * cl[1] + Di[c * 3 + 2] * cl[2];
          }
        }
        pr.T = oplus(pr.T, x.data());
        for (int q = 0; q < n; ++q) for (int c = 0; c < 3; ++c) pr.pts[q].X[c] += x[6 + 3 * q + c];
        double tempChi = pr.chi2();
        if (!ok2) tempChi = std::numeric_limits<double>::max();
        double scale = 0;
        for (int k = 0; k < N; ++k) scale += x[k] * (lambda * x[k] + b[k]);
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
          pr = backup;
        }
        ++qmax; ++trials;
      } while (rho < 0 && qmax < 10);
      chiLast = currentChi;
      if (qmax == 10 || rho == 0 || rho != rho) break;
      if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
      if (nBad >= 3) break;
    }
  }
  // write-back in float, median depth in keyframe 1, scaling, UpdateNormalAndDepth
  float Tf[12];
  for (int k = 0; k < 9; ++k) Tf[k] = (float)pr.T.R[k];
  for (int k = 0; k < 3; ++k) Tf[9 + k] = (float)pr.T.t[k];
  std::vector<float> pos((size_t)3 * n), depths;
  for (int q = 0; q < n; ++q) { for (int c = 0; c < 3; ++c) pos[3 * q + c] = (float)pr.pts[q].X[c]; depths.push_back(pos[3 * q + 2]); }
  float med = -1.f;
  if (n > 0) { std::sort(depths.begin(), depths.end()); med = depths[(depths.size() - 1) / 2]; }
  int status = 0;
  if (med < 0) status |= 2;
  if (n < minTracked) status |= 4;
  if (!status) status = 1;
  const float inv = depthScale / med;
  const bool scaleIt = status == 1 && depthScale != 0.f;
  if (scaleIt) for (int k = 0; k < 3; ++k) Tf[9 + k] *= inv;
  float Ow2[3];
  for (int i = 0; i < 3; ++i) Ow2[i] = -(Tf[i] * Tf[9] + Tf[3 + i] * Tf[10] + Tf[6 + i] * Tf[11]);
  for (int q = 0; q < n; ++q) {
    float* X = &pos[3 * q];
    if (scaleIt) for (int c = 0; c < 3; ++c) X[c] *= inv;
    const float a[3] = {X[0], X[1], X[2]}, bb[3] = {X[0] - Ow2[0], X[1] - Ow2[1], X[2] - Ow2[2]};
    const float la = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), lb = std::sqrt(bb[0] * bb[0] + bb[1] * bb[1] + bb[2] * bb[2]);
    const int i = pr.pts[q].i, j = pr.pts[q].j;
    for (int c = 0; c < 3; ++c) { mpPos[3 * i + c] = X[c]; mpNormal[3 * i + c] = (a[c] / la + bb[c] / lb) / 2; }
    mpDist[2 * i] = lb * scaleFactors[(int)kp2[3 * j + 2]];
    mpDist[2 * i + 1] = mpDist[2 * i] / scaleFactors[nlevels - 1];
    hasMP[i] = 1;
  }
  memcpy(Tcw2, Tf, 48);
  stats[0] = n; stats[1] = its; stats[2] = trials; stats[3] = stopSeen;
  chi2[0] = chiFirst; chi2[1] = chiLast;
  *median = med;
  return status;
}

}  // extern "C"
