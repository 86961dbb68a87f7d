// CPU oracle of MLPnPsolver (reference src/MLPnPsolver.cpp): an independent restatement of the class with plain arrays and the
// host libm, built by tests/mlpnp_solver_oracle.py with g++ -O2 -ffp-contract=off and loaded with ctypes.
// It shares with the kernel only the conventions of DESIGN.md section 6 ("MLPnPsolver"):
//   * null-space basis of a bearing vector f: u = f / |f|, a = 1 / (1 + u_z), b = -u_x u_y a, r = (1 - u_x^2 a, b, -u_x),
//     s = (b, 1 - u_y^2 a, -u_y);
//   * every sum over correspondences (P P^T, A^T A, J^T J, J^T r) runs in list order into one accumulator per entry, row r then row s;
//   * symmetric eigenproblems (12 x 12, 9 x 9, 3 x 3) by one FP64 cyclic Jacobi: pairs (p, q) row by row, rotations skipped when
//     a_pq == 0, the symmetric one-pass update, stop when not (off > 1e-30 * fro), at most 30 sweeps, off and fro summed by columns;
//   * the null vector = the eigenvector of the first smallest |eigenvalue|;
//   * rank of P P^T = the number of |eigenvalues| above 3 * 2^-52 * the largest; eigenframe = eigenvectors by increasing eigenvalue
//     (ties by index), signs as Jacobi leaves them;
//   * nearest rotation of M = M V diag(lambda^-1/2) V^T with (lambda, V) of M^T M, negated when its determinant is negative;
//   * general case translation candidates -s t and +s t (the inverse of [R | +-R s t] taken in closed form);
//   * 6 x 6 LDL^T without pivoting; a NaN in dx leaves the Gauss-Newton loop;
//   * d(R(w) X)/dw = -R [X]x (w w^T + (R^T - I) [w]x) / |w|^2, and -[X]x when |w| <= 1e-8.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct Camera {
  bool kb8;
  float p[8];
  void unproject(float px, float py, float* ray) const {   // Pinhole::unproject / KannalaBrandt8::unproject
    if (!kb8) {
      ray[0] = (px - p[2]) / p[0];
      ray[1] = (py - p[3]) / p[1];
      ray[2] = 1.f;
      return;
    }
    const float pwx = (px - p[2]) / p[0], pwy = (py - p[3]) / p[1];
    float scale = 1.f;
    float theta_d = sqrtf(pwx * pwx + pwy * pwy);
    theta_d = fminf(fmaxf((float)(-M_PI / 2.f), theta_d), (float)(M_PI / 2.f));
    if (theta_d > 1e-8f) {
      float theta = theta_d;
      for (int j = 0; j < 10; j++) {
        const float theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta4 * theta4;
        const float k0 = p[4] * theta2, k1 = p[5] * theta4, k2 = p[6] * theta6, k3 = p[7] * theta8;
        const float fix = (theta * (1 + k0 + k1 + k2 + k3) - theta_d) / (1 + 3 * k0 + 5 * k1 + 7 * k2 + 9 * k3);
        theta = theta - fix;
        if (fabsf(fix) < 1e-6f) break;
      }
      scale = tanf(theta) / theta_d;
    }
    ray[0] = pwx * scale;
    ray[1] = pwy * scale;
    ray[2] = 1.f;
  }
  void project(const float* v, float* uv) const {   // project(cv::Point3f)
    if (!kb8) {
      uv[0] = p[0] * v[0] / v[2] + p[2];
      uv[1] = p[1] * v[1] / v[2] + p[3];
      return;
    }
    const float x2_plus_y2 = v[0] * v[0] + v[1] * v[1];
    const float theta = atan2f(sqrtf(x2_plus_y2), v[2]);
    const float psi = atan2f(v[1], v[0]);
    const float theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta3 * theta2, theta7 = theta5 * theta2, theta9 = theta7 * theta2;
    const float r = theta + p[4] * theta3 + p[5] * theta5 + p[6] * theta7 + p[7] * theta9;
    uv[0] = p[0] * r * cosf(psi) + p[2];
    uv[1] = p[1] * r * sinf(psi) + p[3];
  }
};

// cyclic Jacobi of the symmetric m x m matrix a (row-major); v receives the eigenvectors as columns, the diagonal of a the eigenvalues
void jacobi(int m, double* a, double* v) {
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) v[i * m + j] = i == j ? 1.0 : 0.0;
  double fro = 0;
  for (int j = 0; j < m; ++j) {
    double c = 0;
    for (int i = 0; i < m; ++i) c += a[i * m + j] * a[i * m + j];
    fro += c;
  }
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0;
    for (int j = 0; j < m; ++j) {
      double c = 0;
      for (int i = 0; i < j; ++i) c += a[i * m + j] * a[i * m + j];
      off += c;
    }
    if (!(off > 1e-30 * fro)) break;
    for (int p = 0; p < m - 1; ++p)
      for (int q = p + 1; q < m; ++q) {
        const double apq = a[p * m + q];
        if (apq == 0.0) continue;
        const double app = a[p * m + p], aqq = a[q * m + q];
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < m; ++k) {
          if (k != p && k != q) {
            const double akp = a[k * m + p], akq = a[k * m + q];
            const double np_ = c * akp - s * akq, nq = s * akp + c * akq;
            a[k * m + p] = np_; a[p * m + k] = np_;
            a[k * m + q] = nq; a[q * m + k] = nq;
          }
          const double vkp = v[k * m + p], vkq = v[k * m + q];
          v[k * m + p] = c * vkp - s * vkq;
          v[k * m + q] = s * vkp + c * vkq;
        }
        a[p * m + p] = app - t * apq;
        a[q * m + q] = aqq + t * apq;
        a[p * m + q] = 0.0;
        a[q * m + p] = 0.0;
      }
  }
}

double det3(const double M[3][3]) {
  return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
         M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

// U V^T of the SVD of M, i.e. M (M^T M)^-1/2; negated when the determinant is negative
void nearest_rotation(const double M[3][3], double R[3][3]) {
  double B[9], V[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) B[i * 3 + j] = M[0][i] * M[0][j] + M[1][i] * M[1][j] + M[2][i] * M[2][j];
  jacobi(3, B, V);
  double S[3][3];
  const double w[3] = {1.0 / std::sqrt(B[0]), 1.0 / std::sqrt(B[4]), 1.0 / std::sqrt(B[8])};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) S[i][j] = V[i * 3] * w[0] * V[j * 3] + V[i * 3 + 1] * w[1] * V[j * 3 + 1] + V[i * 3 + 2] * w[2] * V[j * 3 + 2];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i][j] = M[i][0] * S[0][j] + M[i][1] * S[1][j] + M[i][2] * S[2][j];
  if (det3(R) < 0)
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) R[i][j] = -R[i][j];
}

void null_basis(const double* f, double N[3][2]) {
  const double n = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
  const double ux = f[0] / n, uy = f[1] / n, uz = f[2] / n;
  const double a = 1.0 / (1.0 + uz), b = -ux * uy * a;
  N[0][0] = 1.0 - ux * ux * a; N[1][0] = b; N[2][0] = -ux;
  N[0][1] = b; N[1][1] = 1.0 - uy * uy * a; N[2][1] = -uy;
}

void rodrigues2rot(const double* w, double R[3][3]) {   // :660-675
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i][j] = i == j ? 1.0 : 0.0;
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  if (th > 2.220446049250313e-16) {
    const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
    const double a = std::sin(th) / th, b = (1 - std::cos(th)) / (th * th);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const double k2 = K[i][0] * K[0][j] + K[i][1] * K[1][j] + K[i][2] * K[2][j];
        R[i][j] = R[i][j] + a * K[i][j] + b * k2;
      }
  }
}

void rot2rodrigues(const double R[3][3], double* w) {   // :677-692
  w[0] = w[1] = w[2] = 0.0;
  const double trace = R[0][0] + R[1][1] + R[2][2] - 1.0;
  const double wnorm = std::acos(trace / 2.0);
  if (wnorm > 2.220446049250313e-16) {
    const double sc = wnorm / (2.0 * std::sin(wnorm));
    w[0] = (R[2][1] - R[1][2]) * sc;
    w[1] = (R[0][2] - R[2][0]) * sc;
    w[2] = (R[1][0] - R[0][1]) * sc;
  }
}

// residual r = N^T normalize(R(w) X + T) and its Jacobian with respect to (w, T), derived by hand:
//   p = R X + T, y = p / |p|, dy/dp = (I - y y^T) / |p|, dp/dT = I,
//   dp/dw = -R [X]x (w w^T + (R^T - I) [w]x) / |w|^2   (-[X]x in the limit |w| -> 0, used for |w| <= 1e-8)
void residual_jac(const double* x, const double R[3][3], const double* X, const double N[3][2], double* r, double J[2][6]) {
  double p[3], y[3];
  for (int i = 0; i < 3; ++i) p[i] = R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + x[3 + i];
  const double n = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  for (int i = 0; i < 3; ++i) y[i] = p[i] / n;
  for (int c = 0; c < 2; ++c) r[c] = N[0][c] * y[0] + N[1][c] * y[1] + N[2][c] * y[2];
  // G = dp/dw
  double G[3][3];
  const double th2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
  const double Xx[3][3] = {{0.0, -X[2], X[1]}, {X[2], 0.0, -X[0]}, {-X[1], X[0], 0.0}};
  if (std::sqrt(th2) <= 1e-8) {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) G[i][j] = -Xx[i][j];
  } else {
    const double Wx[3][3] = {{0.0, -x[2], x[1]}, {x[2], 0.0, -x[0]}, {-x[1], x[0], 0.0}};
    double Q[3][3], RX[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += (R[k][i] - (k == i ? 1.0 : 0.0)) * Wx[k][j];
        Q[i][j] = (x[i] * x[j] + s) / th2;
        RX[i][j] = R[i][0] * Xx[0][j] + R[i][1] * Xx[1][j] + R[i][2] * Xx[2][j];
      }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) G[i][j] = -(RX[i][0] * Q[0][j] + RX[i][1] * Q[1][j] + RX[i][2] * Q[2][j]);
  }
  // rows of N^T (I - y y^T) / n
  for (int c = 0; c < 2; ++c) {
    double d[3];
    for (int j = 0; j < 3; ++j) d[j] = (N[j][c] - r[c] * y[j]) / n;
    for (int j = 0; j < 3; ++j) {
      J[c][j] = d[0] * G[0][j] + d[1] * G[1][j] + d[2] * G[2][j];
      J[c][3 + j] = d[j];
    }
  }
}

bool ldlt6_solve(double A[6][6], const double* g, double* x) {   // no pivoting; false when a value is not finite
  double L[6][6] = {}, D[6];
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k] * D[k];
    D[j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k] * D[k];
      L[i][j] = s / d;
    }
  }
  double z[6];
  for (int i = 0; i < 6; ++i) {
    double s = g[i];
    for (int k = 0; k < i; ++k) s -= L[i][k] * z[k];
    z[i] = s;
  }
  for (int i = 5; i >= 0; --i) {
    double s = z[i] / D[i];
    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * x[k];
    x[i] = s;
  }
  for (int i = 0; i < 6; ++i)
    if (!(std::fabs(x[i]) <= 1.79769313486231570815e308)) return false;
  return true;
}

struct Solver {
  Camera cam;
  int nFeatures = 0;
  std::vector<double> f, X;   // [N][3]
  std::vector<float> p2d, sigma2, maxError;
  std::vector<int> keyIdx;
  int N = 0;
  double prob = 0;
  int minInliers = 0, maxIts = 0, minSet = 6;
  float epsilon = 0;
  int nIterations = 0;
  double Ri[3][3], ti[3];
  std::vector<uint8_t> inliersi, bestInliers, refinedInliers;
  int nInliersi = 0, nBest = 0, nRefined = 0;
  float bestTcw[16], refinedTcw[16];
  bool refineCurrent = false;   // a test knob: Refine() on the current mask instead of the best one (NOT the reference)

  void setRansacParameters(double probability, int minIn, int maxIterations, int minSet_, float eps, float th2) {
    prob = probability; minInliers = minIn; maxIts = maxIterations; epsilon = eps; minSet = minSet_;
    N = (int)p2d.size() / 2;
    inliersi.assign(N, 0);
    int nMin = N * epsilon;
    if (nMin < minInliers) nMin = minInliers;
    if (nMin < minSet) nMin = minSet;
    minInliers = nMin;
    if (epsilon < (float)minInliers / N) epsilon = (float)minInliers / N;
    int nIt;
    if (minInliers == N) nIt = 1;
    else nIt = ceil(log(1 - prob) / log(1 - pow(epsilon, 3)));
    maxIts = std::max(1, std::min(nIt, maxIts));
    maxError.resize(N);
    for (int i = 0; i < N; ++i) maxError[i] = sigma2[i] * th2;
  }

  void checkInliers() {
    nInliersi = 0;
    for (int i = 0; i < N; ++i) {
      const double* Xi = &X[3 * i];
      float Pc[3], uv[2];
      const float x = (float)Xi[0], y = (float)Xi[1], z = (float)Xi[2];
      for (int r = 0; r < 3; ++r) Pc[r] = (float)(Ri[r][0] * x + Ri[r][1] * y + Ri[r][2] * z + ti[r]);
      cam.project(Pc, uv);
      const float dx = p2d[2 * i] - uv[0], dy = p2d[2 * i + 1] - uv[1];
      const float e2 = dx * dx + dy * dy;
      inliersi[i] = e2 < maxError[i];
      nInliersi += inliersi[i];
    }
  }

  void computePose(const std::vector<int>& idx) {
    const int n = (int)idx.size();
    std::vector<double> Ns(n * 6);
    double M[9] = {};
    for (int k = 0; k < n; ++k) {
      double Nk[3][2];
      null_basis(&f[3 * idx[k]], Nk);
      for (int a = 0; a < 3; ++a) { Ns[k * 6 + a * 2] = Nk[a][0]; Ns[k * 6 + a * 2 + 1] = Nk[a][1]; }
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double s = 0;
        for (int k = 0; k < n; ++k) s += X[3 * idx[k] + i] * X[3 * idx[k] + j];
        M[i * 3 + j] = s;
      }
    double E[9], lam[9];
    memcpy(lam, M, sizeof M);
    jacobi(3, lam, E);
    const double ev[3] = {lam[0], lam[4], lam[8]};
    double big = 0;
    for (int k = 0; k < 3; ++k) big = std::fabs(ev[k]) > big ? std::fabs(ev[k]) : big;
    int rank = 0;
    for (int k = 0; k < 3; ++k) rank += std::fabs(ev[k]) > big * 2.220446049250313e-16 * 3.0;
    const bool planar = rank == 2;
    double Er[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};   // eigenRot: rows = eigenvectors by increasing eigenvalue
    if (planar) {
      int ord[3] = {0, 1, 2};
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2 - a; ++b)
          if (ev[ord[b + 1]] < ev[ord[b]]) std::swap(ord[b], ord[b + 1]);
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Er[r][c] = E[c * 3 + ord[r]];
    }
    const int m = planar ? 9 : 12;
    std::vector<double> A(m * m, 0.0), V(m * m);
    for (int c2 = 0; c2 < m; ++c2)
      for (int c1 = 0; c1 <= c2; ++c1) {
        double s = 0;
        for (int k = 0; k < n; ++k) {
          const double* Xk = &X[3 * idx[k]];
          double Y[3];
          for (int r = 0; r < 3; ++r) Y[r] = planar ? Er[r][0] * Xk[0] + Er[r][1] * Xk[1] + Er[r][2] * Xk[2] : Xk[r];
          for (int row = 0; row < 2; ++row) {
            auto entry = [&](int c) {
              if (planar) return c < 6 ? Ns[k * 6 + (c / 2) * 2 + row] * Y[1 + c % 2] : Ns[k * 6 + (c - 6) * 2 + row];
              return c < 9 ? Ns[k * 6 + (c / 3) * 2 + row] * Y[c % 3] : Ns[k * 6 + (c - 9) * 2 + row];
            };
            s += entry(c1) * entry(c2);
          }
        }
        A[c1 * m + c2] = s;
        A[c2 * m + c1] = s;
      }
    jacobi(m, A.data(), V.data());
    int kmin = 0;
    for (int k = 1; k < m; ++k)
      if (std::fabs(A[k * m + k]) < std::fabs(A[kmin * m + kmin])) kmin = k;
    double x[12];
    for (int k = 0; k < m; ++k) x[k] = V[k * m + kmin];
    double Rout[3][3], tout[3];
    auto repro = [&](const double R[3][3], const double* t) {   // over the first six correspondences, un-normalised bearing vectors
      double s = 0;
      for (int p = 0; p < 6; ++p) {
        const double* Xp = &X[3 * idx[p]];
        const double* fp = &f[3 * idx[p]];
        double v[3];
        for (int r = 0; r < 3; ++r) v[r] = R[r][0] * Xp[0] + R[r][1] * Xp[1] + R[r][2] * Xp[2] + t[r];
        const double nv = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        s += 1.0 - (v[0] / nv * fp[0] + v[1] / nv * fp[1] + v[2] / nv * fp[2]);
      }
      return s;
    };
    if (planar) {
      double T[3][3];   // rows: c1 x c2, c1, c2 with c1 = (x0 x2 x4), c2 = (x1 x3 x5)
      const double c1[3] = {x[0], x[2], x[4]}, c2[3] = {x[1], x[3], x[5]};
      T[0][0] = c1[1] * c2[2] - c1[2] * c2[1];
      T[0][1] = c1[2] * c2[0] - c1[0] * c2[2];
      T[0][2] = c1[0] * c2[1] - c1[1] * c2[0];
      for (int a = 0; a < 3; ++a) { T[1][a] = c1[a]; T[2][a] = c2[a]; }
      const double n1 = std::sqrt(T[0][1] * T[0][1] + T[1][1] * T[1][1] + T[2][1] * T[2][1]);
      const double n2 = std::sqrt(T[0][2] * T[0][2] + T[1][2] * T[1][2] + T[2][2] * T[2][2]);
      const double scale = 1.0 / std::sqrt(std::fabs(n1 * n2));
      double Rn[3][3], R1[3][3], R2[3][3];
      nearest_rotation(T, Rn);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          const double back = Er[0][j] * Rn[0][i] + Er[1][j] * Rn[1][i] + Er[2][j] * Rn[2][i];   // (eigenRot^T Rn)(j, i)
          R1[i][j] = -back;
        }
      if (det3(R1) < 0)
        for (int i = 0; i < 3; ++i) R1[i][2] = -R1[i][2];
      for (int i = 0; i < 3; ++i) { R2[i][0] = -R1[i][0]; R2[i][1] = -R1[i][1]; R2[i][2] = R1[i][2]; }
      const double t[3] = {scale * x[6], scale * x[7], scale * x[8]}, tn[3] = {-t[0], -t[1], -t[2]};
      const double nv[4] = {repro(R1, t), repro(R1, tn), repro(R2, t), repro(R2, tn)};
      int best = 0;
      for (int k = 1; k < 4; ++k)
        if (nv[k] < nv[best]) best = k;
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Rout[i][j] = best < 2 ? R1[i][j] : R2[i][j];
        tout[i] = (best & 1) ? tn[i] : t[i];
      }
    } else {
      double Mt[3][3], Rn[3][3];   // Mt = the reference's tmp: the transpose of the row-major 3 x 3 of x
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Mt[i][j] = x[3 * j + i];
      double cn[3];
      for (int j = 0; j < 3; ++j) cn[j] = std::sqrt(Mt[0][j] * Mt[0][j] + Mt[1][j] * Mt[1][j] + Mt[2][j] * Mt[2][j]);
      const double scale = 1.0 / std::cbrt(std::fabs(cn[0] * cn[1] * cn[2]));
      nearest_rotation(Mt, Rn);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rout[i][j] = Rn[j][i];
      const double tp[3] = {scale * x[9], scale * x[10], scale * x[11]}, tm[3] = {-tp[0], -tp[1], -tp[2]};
      const double e0 = repro(Rout, tm), e1 = repro(Rout, tp);
      for (int i = 0; i < 3; ++i) tout[i] = e0 < e1 ? tm[i] : tp[i];
    }
    // Gauss-Newton (:694-758)
    double xs[6];
    rot2rodrigues(Rout, xs);
    for (int i = 0; i < 3; ++i) xs[3 + i] = tout[i];
    for (int it = 0; it < 5; ++it) {
      double R[3][3];
      rodrigues2rot(xs, R);
      double JtJ[6][6] = {}, g[6] = {};
      for (int k = 0; k < n; ++k) {
        double Nk[3][2] = {{Ns[k * 6], Ns[k * 6 + 1]}, {Ns[k * 6 + 2], Ns[k * 6 + 3]}, {Ns[k * 6 + 4], Ns[k * 6 + 5]}};
        double r[2], J[2][6];
        residual_jac(xs, R, &X[3 * idx[k]], Nk, r, J);
        for (int row = 0; row < 2; ++row)
          for (int a = 0; a < 6; ++a) {
            for (int b = 0; b < 6; ++b) JtJ[a][b] += J[row][a] * J[row][b];
            g[a] += J[row][a] * r[row];
          }
      }
      double dx[6];
      if (!ldlt6_solve(JtJ, g, dx)) break;
      double mx = 0, mn = 1e300;
      for (int a = 0; a < 6; ++a) { mx = std::max(mx, std::fabs(dx[a])); mn = std::min(mn, std::fabs(dx[a])); }
      if (mx > 5.0 || mn > 1.0) break;
      double dl = 0;
      for (int k = 0; k < n; ++k) {
        double Nk[3][2] = {{Ns[k * 6], Ns[k * 6 + 1]}, {Ns[k * 6 + 2], Ns[k * 6 + 3]}, {Ns[k * 6 + 4], Ns[k * 6 + 5]}};
        double r[2], J[2][6];
        residual_jac(xs, R, &X[3 * idx[k]], Nk, r, J);
        for (int row = 0; row < 2; ++row) {
          double s = 0;
          for (int a = 0; a < 6; ++a) s += J[row][a] * dx[a];
          dl = std::max(dl, std::fabs(s));
        }
      }
      for (int a = 0; a < 6; ++a) xs[a] -= dx[a];
      if (dl < 1e-5) break;
    }
    rodrigues2rot(xs, Ri);
    for (int i = 0; i < 3; ++i) ti[i] = xs[3 + i];
  }

  void toFloat(float* T) const {
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.f : 0.f;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) T[r * 4 + c] = (float)Ri[r][c];
      T[r * 4 + 3] = (float)ti[r];
    }
  }

  bool refine() {
    std::vector<int> idx;
    const std::vector<uint8_t>& src = refineCurrent ? inliersi : bestInliers;
    const std::vector<uint8_t> copy = src;
    for (size_t i = 0; i < copy.size(); ++i)
      if (copy[i]) idx.push_back((int)i);
    computePose(idx);
    checkInliers();
    nRefined = nInliersi;
    refinedInliers = inliersi;
    if (nInliersi > minInliers) { toFloat(refinedTcw); return true; }
    return false;
  }

  // one call of iterate(n, bNoMore, vbInliers, nInliers, Tout); res: ok noMore nInliers iterations bestInliers refined returnedAt
  bool iterate(int nIts, const int* rnd, int rndLen, int* hyp, int hypCap, int* res, float* Tout, uint8_t* mask) {
    for (int k = 0; k < 16; ++k) Tout[k] = (k % 5 == 0) ? 1.f : 0.f;
    memset(mask, 0, nFeatures);
    res[0] = res[1] = res[2] = 0; res[5] = 0; res[6] = -1;
    auto fin = [&]() { res[3] = nIterations; res[4] = nBest; };
    if (N < minInliers) { res[1] = 1; fin(); return false; }
    int cur = 0;
    while (nIterations < maxIts || cur < nIts) {
      if ((nIterations + 1) * minSet > rndLen) break;   // the recorded rand() stream is spent
      cur++;
      nIterations++;
      const int* r = rnd + (size_t)(nIterations - 1) * minSet;
      std::vector<int> avail(N), idx(minSet);
      for (int i = 0; i < N; ++i) avail[i] = i;
      for (int i = 0; i < minSet; ++i) {
        const int d = (int)avail.size();
        const int randi = int(((double)r[i] / ((double)RAND_MAX + 1.0)) * d);
        idx[i] = avail[randi];
        avail[randi] = avail.back();
        avail.pop_back();
      }
      computePose(idx);
      checkInliers();
      if (nIterations - 1 < hypCap) hyp[nIterations - 1] = nInliersi;
      if (nInliersi >= minInliers) {
        if (nInliersi > nBest) {
          bestInliers = inliersi;
          nBest = nInliersi;
          toFloat(bestTcw);
        }
        if (refine()) {
          res[0] = 1; res[2] = nRefined; res[5] = 1; res[6] = nIterations - 1;
          for (int i = 0; i < N; ++i)
            if (refinedInliers[i]) mask[keyIdx[i]] = 1;
          memcpy(Tout, refinedTcw, sizeof refinedTcw);
          fin();
          return true;
        }
      }
    }
    if (nIterations >= maxIts) {
      res[1] = 1;
      if (nBest >= minInliers) {
        res[0] = 1; res[2] = nBest;
        for (int i = 0; i < N; ++i)
          if (bestInliers[i]) mask[keyIdx[i]] = 1;
        memcpy(Tout, bestTcw, sizeof bestTcw);
        fin();
        return true;
      }
    }
    fin();
    return false;
  }
};

}  // namespace

extern "C" {

// ints: [0] minInliers [1] maxIterations [2] minSet [3] ncalls [4] stop at the first call that returns true or bNoMore [5] the test knob
// Returns the number of calls made; head = N, adjusted minInliers, budget.
int mlpnp_oracle_run(int n, const uint8_t* entry, const float* uv, const float* sigma2, const float* Xw, const float* cam9,
                     double probability, float epsilon, float th2, const int* ints, const int* calls, const int* rnd, int rndLen,
                     int* hyp, int hypCap, int* head, int* res /*[ncalls][7]*/, float* Tcw /*[ncalls][16]*/, float* bestTcw /*[ncalls][16]*/,
                     uint8_t* mask /*[ncalls][n]*/, uint8_t* bestMask /*[ncalls][n]*/) {
  Solver s;
  s.cam.kb8 = cam9[0] != 0.f;
  for (int i = 0; i < 8; ++i) s.cam.p[i] = cam9[1 + i];
  s.nFeatures = n;
  s.refineCurrent = ints[5] != 0;
  for (int i = 0; i < n; ++i) {
    if (!(entry[i] & 1) || (entry[i] & 2) || (entry[i] & 4)) continue;
    float ray[3];
    s.cam.unproject(uv[2 * i], uv[2 * i + 1], ray);
    const float bx = ray[0] / ray[2], by = ray[1] / ray[2], bz = ray[2] / ray[2];
    s.p2d.push_back(uv[2 * i]); s.p2d.push_back(uv[2 * i + 1]);
    s.sigma2.push_back(sigma2[i]);
    s.f.push_back(bx); s.f.push_back(by); s.f.push_back(bz);
    for (int r = 0; r < 3; ++r) s.X.push_back((double)Xw[3 * i + r]);
    s.keyIdx.push_back(i);
  }
  s.setRansacParameters(probability, ints[0], ints[1], ints[2], epsilon, th2);
  head[0] = s.N; head[1] = s.minInliers; head[2] = s.maxIts;
  memset(s.bestTcw, 0, sizeof s.bestTcw);
  int made = 0;
  const int stride = n > 0 ? n : 1;
  for (int c = 0; c < ints[3]; ++c) {
    const bool ok = s.iterate(calls[c], rnd, rndLen, hyp, hypCap, res + 7 * c, Tcw + 16 * c, mask + (size_t)stride * c);
    memcpy(bestTcw + 16 * c, s.bestTcw, sizeof s.bestTcw);
    memset(bestMask + (size_t)stride * c, 0, stride);
    for (size_t i = 0; i < s.bestInliers.size(); ++i)
      if (s.bestInliers[i]) bestMask[(size_t)stride * c + s.keyIdx[i]] = 1;
    ++made;
    if (ints[4] && (ok || res[7 * c + 1])) break;
  }
  return made;
}

// residual and Jacobian of one correspondence at x = (w, T): for the finite-difference check of the hand derivation
void mlpnp_oracle_residual_jac(const double* x, const double* X, const double* f, double* r, double* J12) {
  double R[3][3], N[3][2], J[2][6];
  rodrigues2rot(x, R);
  null_basis(f, N);
  residual_jac(x, R, X, N, r, J);
  for (int c = 0; c < 2; ++c)
    for (int a = 0; a < 6; ++a) J12[c * 6 + a] = J[c][a];
}

void mlpnp_oracle_ransac(int N, int minInliers, int maxIterations, int minSet, float epsilon, double probability, int* out3) {
  Solver s;
  s.p2d.assign(2 * (size_t)N, 0.f);
  s.sigma2.assign(N, 1.f);
  s.setRansacParameters(probability, minInliers, maxIterations, minSet, epsilon, 5.991f);
  out3[0] = s.minInliers; out3[1] = s.maxIts; out3[2] = s.N;
}

}  // extern "C"
