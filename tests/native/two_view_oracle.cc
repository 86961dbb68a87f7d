// CPU oracle of TwoViewReconstruction (reference src/TwoViewReconstruction.cc, GeometricTools::Triangulate of src/GeometricTools.cc:48-72,
// Pinhole::ReconstructWithTwoViews of src/CameraModels/Pinhole.cpp:85-98): an independent restatement with plain arrays and the host libm,
// built by tests/two_view_oracle.py with g++ -O2 -ffp-contract=off and loaded with ctypes.  It shares with the product only
// include/morb/two_view_math.h (the d_stats / d_fstats indices and the two scalar conversions; the sampling here uses the reference's
// vector, the header's form is checked against it) and the conventions of DESIGN.md section 6 ("TwoViewReconstruction"):
//   * every float expression of the reference is kept in float, in its order; 3 x 3 products sum k = 0, 1, 2 left to right; a 3 x 3
//     inverse is the adjugate times 1 / det;
//   * symmetric eigenproblems (9 x 9, 4 x 4, 3 x 3) by one FP64 cyclic Jacobi: pairs (p, q) row by row, rotations skipped when
//     a_pq == 0, the symmetric one-pass update, stop when not (off > 1e-30 * fro), at most 30 sweeps, off and fro summed by columns;
//   * null vector of a float A (8 x 9, 16 x 9, 4 x 4): A^T A in FP64 (each entry summed over the rows in order), the eigenvector of the
//     first smallest |eigenvalue|, rounded to float;
//   * SVD of a float 3 x 3 M: (lambda, V) of M^T M in FP64 by decreasing lambda (ties by index), w = sqrt(max(lambda, 0)),
//     u0 = M v0 / |M v0|, u1 = M v1 less its u0 part, normalised, u2 = u0 x u1, v2 = v0 x v1 (det U = det V = +1) and w2 carries the
//     sign of det M; all rounded to float.  ReconstructH, the one user of w2, moves a negative sign into V's last column;
//   * rank-2 enforcement: Fn(i, j) = (U(i,0) w0) V(j,0) + (U(i,1) w1) V(j,1) in float;
//   * vCosParallax: std::sort, then the element at min(50, size - 1).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "morb/two_view_math.h"

namespace {

using namespace morbtv;

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

// the last right singular vector of the rows x m float matrix A (m <= 9)
void null_vector(const float* A, int rows, int m, float* x) {
  double B[81], V[81];
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) {
      double s = 0;
      for (int r = 0; r < rows; ++r) s += (double)A[r * m + i] * (double)A[r * m + j];
      B[i * m + j] = s;
    }
  jacobi(m, B, V);
  int kmin = 0;
  double best = std::fabs(B[0]);
  for (int k = 1; k < m; ++k) {
    const double v = std::fabs(B[k * m + k]);
    if (v < best) { best = v; kmin = k; }
  }
  for (int k = 0; k < m; ++k) x[k] = (float)V[k * m + kmin];
}

// M = U diag(w) V^T, every matrix row-major
void svd3(const float* M, float* U, float* w, float* Vo) {
  double Md[9], B[9], V[9];
  for (int i = 0; i < 9; ++i) Md[i] = (double)M[i];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) B[i * 3 + j] = Md[i] * Md[j] + Md[3 + i] * Md[3 + j] + Md[6 + i] * Md[6 + j];
  jacobi(3, B, V);
  int o[3] = {0, 1, 2};
  double l[3] = {B[0], B[4], B[8]};
  auto sw = [&](int a, int b) { if (l[b] > l[a]) { std::swap(l[a], l[b]); std::swap(o[a], o[b]); } };
  sw(0, 1); sw(1, 2); sw(0, 1);
  double v[3][3], u[3][3];
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 3; ++i) v[k][i] = V[i * 3 + o[k]];
  double a0[3], a1[3];
  for (int i = 0; i < 3; ++i) {
    a0[i] = Md[i * 3] * v[0][0] + Md[i * 3 + 1] * v[0][1] + Md[i * 3 + 2] * v[0][2];
    a1[i] = Md[i * 3] * v[1][0] + Md[i * 3 + 1] * v[1][1] + Md[i * 3 + 2] * v[1][2];
  }
  const double n0 = std::sqrt(a0[0] * a0[0] + a0[1] * a0[1] + a0[2] * a0[2]);
  for (int i = 0; i < 3; ++i) u[0][i] = a0[i] / n0;
  const double d = u[0][0] * a1[0] + u[0][1] * a1[1] + u[0][2] * a1[2];
  for (int i = 0; i < 3; ++i) a1[i] = a1[i] - d * u[0][i];
  const double n1 = std::sqrt(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]);
  for (int i = 0; i < 3; ++i) u[1][i] = a1[i] / n1;
  u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
  u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
  u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
  v[2][0] = v[0][1] * v[1][2] - v[0][2] * v[1][1];
  v[2][1] = v[0][2] * v[1][0] - v[0][0] * v[1][2];
  v[2][2] = v[0][0] * v[1][1] - v[0][1] * v[1][0];
  double a2[3];
  for (int i = 0; i < 3; ++i) a2[i] = Md[i * 3] * v[2][0] + Md[i * 3 + 1] * v[2][1] + Md[i * 3 + 2] * v[2][2];
  const bool neg = u[2][0] * a2[0] + u[2][1] * a2[1] + u[2][2] * a2[2] < 0;   // det M < 0
  for (int k = 0; k < 3; ++k) {
    w[k] = (float)std::sqrt(l[k] < 0 ? 0.0 : l[k]);
    if (k == 2 && neg) w[k] = -w[k];
    for (int i = 0; i < 3; ++i) { U[i * 3 + k] = (float)u[k][i]; Vo[i * 3 + k] = (float)v[k][i]; }
  }
}

void mul33(const float* A, const float* B, float* C) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
void transpose33(const float* A, float* T) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) T[i * 3 + j] = A[j * 3 + i];
}
float det33(const float* a) {
  return a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
}
void inverse33(const float* a, float* o) {
  const float inv = 1.0f / det33(a);
  o[0] = (a[4] * a[8] - a[5] * a[7]) * inv; o[1] = (a[2] * a[7] - a[1] * a[8]) * inv; o[2] = (a[1] * a[5] - a[2] * a[4]) * inv;
  o[3] = (a[5] * a[6] - a[3] * a[8]) * inv; o[4] = (a[0] * a[8] - a[2] * a[6]) * inv; o[5] = (a[2] * a[3] - a[0] * a[5]) * inv;
  o[6] = (a[3] * a[7] - a[4] * a[6]) * inv; o[7] = (a[1] * a[6] - a[0] * a[7]) * inv; o[8] = (a[0] * a[4] - a[1] * a[3]) * inv;
}

struct Pt { float x, y; };

struct Solver {
  std::vector<Pt> k1, k2;                        // mvKeys1 / mvKeys2 (pt only)
  std::vector<std::pair<int, int>> m12;          // mvMatches12
  std::vector<std::vector<size_t>> sets;         // mvSets
  float K[9], sigma, sigma2;
  int maxIterations;

  // Normalize (:723-768)
  static void normalize(const std::vector<Pt>& keys, std::vector<Pt>& out, float* T) {
    float meanX = 0, meanY = 0;
    const int N = (int)keys.size();
    out.resize(N);
    for (int i = 0; i < N; ++i) { meanX += keys[i].x; meanY += keys[i].y; }
    meanX = meanX / N;
    meanY = meanY / N;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < N; ++i) {
      out[i].x = keys[i].x - meanX;
      out[i].y = keys[i].y - meanY;
      meanDevX += std::fabs(out[i].x);
      meanDevY += std::fabs(out[i].y);
    }
    meanDevX = meanDevX / N;
    meanDevY = meanDevY / N;
    const float sX = 1.0f / meanDevX, sY = 1.0f / meanDevY;   // 1.0 / float, rounded to float: the same value as the float quotient
    for (int i = 0; i < N; ++i) { out[i].x = out[i].x * sX; out[i].y = out[i].y * sY; }
    for (int i = 0; i < 9; ++i) T[i] = 0.f;
    T[0] = sX; T[4] = sY; T[2] = -meanX * sX; T[5] = -meanY * sY; T[8] = 1.f;
  }

  // ComputeH21 (:227-265)
  static void computeH21(const Pt* p1, const Pt* p2, float* H) {
    float A[16 * 9];
    for (int i = 0; i < 8; ++i) {
      const float u1 = p1[i].x, v1 = p1[i].y, u2 = p2[i].x, v2 = p2[i].y;
      float* a = A + 2 * i * 9;
      a[0] = 0.f; a[1] = 0.f; a[2] = 0.f; a[3] = -u1; a[4] = -v1; a[5] = -1.f; a[6] = v2 * u1; a[7] = v2 * v1; a[8] = v2;
      a += 9;
      a[0] = u1; a[1] = v1; a[2] = 1.f; a[3] = 0.f; a[4] = 0.f; a[5] = 0.f; a[6] = -u2 * u1; a[7] = -u2 * v1; a[8] = -u2;
    }
    null_vector(A, 16, 9, H);
  }

  // ComputeF21 (:267-303)
  static void computeF21(const Pt* p1, const Pt* p2, float* F) {
    float A[8 * 9], Fpre[9], U[9], w[3], V[9];
    for (int i = 0; i < 8; ++i) {
      const float u1 = p1[i].x, v1 = p1[i].y, u2 = p2[i].x, v2 = p2[i].y;
      float* a = A + i * 9;
      a[0] = u2 * u1; a[1] = u2 * v1; a[2] = u2; a[3] = v2 * u1; a[4] = v2 * v1; a[5] = v2; a[6] = u1; a[7] = v1; a[8] = 1.f;
    }
    null_vector(A, 8, 9, Fpre);
    svd3(Fpre, U, w, V);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) F[i * 3 + j] = (U[i * 3] * w[0]) * V[j * 3] + (U[i * 3 + 1] * w[1]) * V[j * 3 + 1];
  }

  // CheckHomography (:305-391)
  float checkHomography(const float* H21, const float* H12, std::vector<uint8_t>& in) const {
    const int N = (int)m12.size();
    in.assign(N, 0);
    float score = 0;
    const float th = 5.991f;
    const float invSigmaSquare = 1.0f / (sigma * sigma);
    for (int i = 0; i < N; ++i) {
      bool bIn = true;
      const float u1 = k1[m12[i].first].x, v1 = k1[m12[i].first].y, u2 = k2[m12[i].second].x, v2 = k2[m12[i].second].y;
      const float w2in1inv = 1.0f / (H12[6] * u2 + H12[7] * v2 + H12[8]);
      const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
      const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
      const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
      const float chiSquare1 = squareDist1 * invSigmaSquare;
      if (chiSquare1 > th) bIn = false;
      else score += th - chiSquare1;
      const float w1in2inv = 1.0f / (H21[6] * u1 + H21[7] * v1 + H21[8]);
      const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
      const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
      const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
      const float chiSquare2 = squareDist2 * invSigmaSquare;
      if (chiSquare2 > th) bIn = false;
      else score += th - chiSquare2;
      in[i] = bIn;
    }
    return score;
  }

  // CheckFundamental (:393-471)
  float checkFundamental(const float* F, std::vector<uint8_t>& in) const {
    const int N = (int)m12.size();
    in.assign(N, 0);
    float score = 0;
    const float th = 3.841f, thScore = 5.991f;
    const float invSigmaSquare = 1.0f / (sigma * sigma);
    for (int i = 0; i < N; ++i) {
      bool bIn = true;
      const float u1 = k1[m12[i].first].x, v1 = k1[m12[i].first].y, u2 = k2[m12[i].second].x, v2 = k2[m12[i].second].y;
      const float a2 = F[0] * u1 + F[1] * v1 + F[2];
      const float b2 = F[3] * u1 + F[4] * v1 + F[5];
      const float c2 = F[6] * u1 + F[7] * v1 + F[8];
      const float num2 = a2 * u2 + b2 * v2 + c2;
      const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
      const float chiSquare1 = squareDist1 * invSigmaSquare;
      if (chiSquare1 > th) bIn = false;
      else score += thScore - chiSquare1;
      const float a1 = F[0] * u2 + F[3] * v2 + F[6];
      const float b1 = F[1] * u2 + F[4] * v2 + F[7];
      const float c1 = F[2] * u2 + F[5] * v2 + F[8];
      const float num1 = a1 * u1 + b1 * v1 + c1;
      const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
      const float chiSquare2 = squareDist2 * invSigmaSquare;
      if (chiSquare2 > th) bIn = false;
      else score += thScore - chiSquare2;
      in[i] = bIn;
    }
    return score;
  }

  // GeometricTools::Triangulate (GeometricTools.cc:48-72); false also stands for the point CheckRT then reads unset
  static bool triangulate(float x1, float y1, float x2, float y2, const float* P1, const float* P2, float* x3D) {
    float A[16], h[4];
    for (int j = 0; j < 4; ++j) {
      A[j] = x1 * P1[8 + j] - P1[j];
      A[4 + j] = y1 * P1[8 + j] - P1[4 + j];
      A[8 + j] = x2 * P2[8 + j] - P2[j];
      A[12 + j] = y2 * P2[8 + j] - P2[4 + j];
    }
    null_vector(A, 4, 4, h);
    if (h[3] == 0) return false;
    for (int k = 0; k < 3; ++k) x3D[k] = h[k] / h[3];
    return true;
  }

  // CheckRT (:770-880)
  int checkRT(const float* R, const float* t, const std::vector<uint8_t>& inl, std::vector<float>& P3D, float th2, std::vector<uint8_t>& good,
              float& parallax) const {
    const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    good.assign(k1.size(), 0);
    P3D.assign(k1.size() * 3, 0.f);
    std::vector<float> vCos;
    float P1[12], P2[12], Rt[12];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j) { P1[i * 4 + j] = j < 3 ? K[i * 3 + j] : 0.f; Rt[i * 4 + j] = j < 3 ? R[i * 3 + j] : t[i]; }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j) P2[i * 4 + j] = K[i * 3] * Rt[j] + K[i * 3 + 1] * Rt[4 + j] + K[i * 3 + 2] * Rt[8 + j];
    float O2[3];
    for (int i = 0; i < 3; ++i) O2[i] = (-R[i]) * t[0] + (-R[3 + i]) * t[1] + (-R[6 + i]) * t[2];
    int nGood = 0;
    for (size_t i = 0; i < m12.size(); ++i) {
      if (!inl[i]) continue;
      const Pt &kp1 = k1[m12[i].first], &kp2 = k2[m12[i].second];
      float p[3];
      if (!triangulate(kp1.x, kp1.y, kp2.x, kp2.y, P1, P2, p)) continue;
      if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;
      const float dist1 = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
      const float n2[3] = {p[0] - O2[0], p[1] - O2[1], p[2] - O2[2]};
      const float dist2 = std::sqrt(n2[0] * n2[0] + n2[1] * n2[1] + n2[2] * n2[2]);
      const float cosParallax = (p[0] * n2[0] + p[1] * n2[1] + p[2] * n2[2]) / (dist1 * dist2);
      if (p[2] <= 0 && (double)cosParallax < 0.99998) continue;
      float q[3];
      for (int r = 0; r < 3; ++r) q[r] = R[r * 3] * p[0] + R[r * 3 + 1] * p[1] + R[r * 3 + 2] * p[2] + t[r];
      if (q[2] <= 0 && (double)cosParallax < 0.99998) continue;
      const float invZ1 = 1.0f / p[2];
      const float im1x = fx * p[0] * invZ1 + cx, im1y = fy * p[1] * invZ1 + cy;
      const float squareError1 = (im1x - kp1.x) * (im1x - kp1.x) + (im1y - kp1.y) * (im1y - kp1.y);
      if (squareError1 > th2) continue;
      const float invZ2 = 1.0f / q[2];
      const float im2x = fx * q[0] * invZ2 + cx, im2y = fy * q[1] * invZ2 + cy;
      const float squareError2 = (im2x - kp2.x) * (im2x - kp2.x) + (im2y - kp2.y) * (im2y - kp2.y);
      if (squareError2 > th2) continue;
      vCos.push_back(cosParallax);
      for (int r = 0; r < 3; ++r) P3D[(size_t)m12[i].first * 3 + r] = p[r];
      nGood++;
      if ((double)cosParallax < 0.99998) good[m12[i].first] = 1;
    }
    if (nGood > 0) {
      std::sort(vCos.begin(), vCos.end());
      const size_t idx = std::min(TV_PARALLAX_RANK, int(vCos.size() - 1));
      parallax = tv_parallax_deg(acosf(vCos[idx]));
    } else
      parallax = 0;
    return nGood;
  }
};

}  // namespace

extern "C" {

void two_view_oracle_null_vector(const float* A, int rows, int m, float* x) { null_vector(A, rows, m, x); }
void two_view_oracle_svd3(const float* M, float* U, float* w, float* V) { svd3(M, U, w, V); }
void two_view_oracle_inverse33(const float* M, float* o) { inverse33(M, o); }

// the sets of :78-95 for N matches; sets [maxIterations][8]
void two_view_oracle_sets(int N, int maxIterations, const int* rnd, int* sets) {
  std::vector<size_t> all, avail;
  for (int i = 0; i < N; ++i) all.push_back(i);
  for (int it = 0; it < maxIterations; ++it) {
    avail = all;
    for (int j = 0; j < 8; ++j) {
      const int d = (int)avail.size() - 1 - 0 + 1;
      const int randi = int(((double)rnd[it * 8 + j] / ((double)2147483647 + 1.0)) * d) + 0;   // DUtils::Random::RandomInt(0, size - 1)
      sets[it * 8 + j] = (int)avail[randi];
      avail[randi] = avail.back();
      avail.pop_back();
    }
  }
}

// Reconstruct (:41-130) on keypoints kp1 [n1][2] / kp2 [n2][2], vMatches12 [n1], K4 = fx fy cx cy.  rnd: 8 rand() values per iteration.
// Outputs: T21 [12] (R row-major, t), P3D [n1][3], tri [n1], stats [TV_STATS_LEN], fstats [TV_FSTATS_LEN], inlH / inlF [n1] by match,
// hyp [2][maxIterations] (the score of every iteration, H then F).  Returns what Reconstruct returns.
int two_view_oracle_run(int n1, int n2, const float* kp1, const float* kp2, const int* matches12, const float* K4, float sigma, int maxIterations,
                        const int* rnd, float* T21, float* P3D, uint8_t* tri, int* stats, float* fstats, uint8_t* inlH, uint8_t* inlF,
                        float* hyp) {
  Solver S;
  for (int i = 0; i < 9; ++i) S.K[i] = 0.f;
  S.K[0] = K4[0]; S.K[4] = K4[1]; S.K[2] = K4[2]; S.K[5] = K4[3]; S.K[8] = 1.f;
  S.sigma = sigma; S.sigma2 = sigma * sigma; S.maxIterations = maxIterations;
  S.k1.resize(n1); S.k2.resize(n2);
  for (int i = 0; i < n1; ++i) S.k1[i] = Pt{kp1[i * 2], kp1[i * 2 + 1]};
  for (int i = 0; i < n2; ++i) S.k2[i] = Pt{kp2[i * 2], kp2[i * 2 + 1]};
  for (int i = 0; i < n1; ++i)
    if (matches12[i] >= 0 && matches12[i] < n2) S.m12.push_back(std::make_pair(i, matches12[i]));   // an entry beyond mvKeys2 is no match

  const int N = (int)S.m12.size();
  for (int i = 0; i < TV_STATS_LEN; ++i) stats[i] = 0;
  for (int i = 0; i < TV_FSTATS_LEN; ++i) fstats[i] = 0.f;
  for (int i = 0; i < 12; ++i) T21[i] = 0.f;
  for (int i = 0; i < n1; ++i) { tri[i] = 0; inlH[i] = 0; inlF[i] = 0; P3D[i * 3] = P3D[i * 3 + 1] = P3D[i * 3 + 2] = 0.f; }
  stats[TV_S_N] = N; stats[TV_S_BEST_IT_H] = -1; stats[TV_S_BEST_IT_F] = -1; stats[TV_S_CHOSEN] = -1;
  if (N < 8) { stats[TV_S_FAIL] = TV_FAIL_FEW_MATCHES; return 0; }
  std::vector<int> sets((size_t)maxIterations * 8);
  two_view_oracle_sets(N, maxIterations, rnd, sets.data());

  std::vector<Pt> n1p, n2p;
  float T1[9], T2[9], T2inv[9], T2t[9];
  Solver::normalize(S.k1, n1p, T1);
  Solver::normalize(S.k2, n2p, T2);
  inverse33(T2, T2inv);
  transpose33(T2, T2t);

  // FindHomography (:132-177) and FindFundamental (:179-225)
  float SH = 0, SF = 0, H[9] = {0}, F[9] = {0};
  std::vector<uint8_t> bestH(N, 0), bestF(N, 0), cur;
  for (int it = 0; it < maxIterations; ++it) {
    Pt a[8], b[8];
    for (int j = 0; j < 8; ++j) {
      const int idx = sets[it * 8 + j];
      a[j] = n1p[S.m12[idx].first];
      b[j] = n2p[S.m12[idx].second];
    }
    float Hn[9], tmp[9], H21i[9], H12i[9], Fn[9], F21i[9];
    Solver::computeH21(a, b, Hn);
    mul33(T2inv, Hn, tmp);
    mul33(tmp, T1, H21i);
    inverse33(H21i, H12i);
    const float sh = S.checkHomography(H21i, H12i, cur);
    hyp[it] = sh;
    if (sh > SH) { memcpy(H, H21i, sizeof H); bestH = cur; SH = sh; stats[TV_S_BEST_IT_H] = it; }
    Solver::computeF21(a, b, Fn);
    mul33(T2t, Fn, tmp);
    mul33(tmp, T1, F21i);
    const float sf = S.checkFundamental(F21i, cur);
    hyp[maxIterations + it] = sf;
    if (sf > SF) { memcpy(F, F21i, sizeof F); bestF = cur; SF = sf; stats[TV_S_BEST_IT_F] = it; }
  }
  for (int i = 0; i < N; ++i) { inlH[i] = bestH[i]; inlF[i] = bestF[i]; }
  fstats[TV_F_SH] = SH; fstats[TV_F_SF] = SF;
  for (int i = 0; i < 9; ++i) { fstats[TV_F_H21_0 + i] = H[i]; fstats[TV_F_F21_0 + i] = F[i]; }
  if (SH + SF == 0.f) { stats[TV_S_FAIL] = TV_FAIL_ZERO_SCORE; return 0; }
  const float RH = SH / (SH + SF);
  fstats[TV_F_RH] = RH;
  const float minParallax = TV_MIN_PARALLAX;
  const int minTriangulated = TV_MIN_TRIANGULATED;
  const float th2 = (float)(4.0 * S.sigma2);
  std::vector<float> vP3D[8];
  std::vector<uint8_t> vGood[8];
  float Rs[8][9], ts[8][3], parallax[8] = {0};
  int nGood[8] = {0};
  int chosen = -1;
  if (RH > 0.50) {   // ReconstructH (:562-721)
    stats[TV_S_MODEL] = 1;
    int Nin = 0;
    for (int i = 0; i < N; ++i) Nin += bestH[i];
    stats[TV_S_NINLIERS] = Nin;
    float invK[9], tmp[9], A[9], U[9], V[9], Vt[9], w[3];
    inverse33(S.K, invK);
    mul33(invK, H, tmp);
    mul33(tmp, S.K, A);
    svd3(A, U, w, V);
    if (w[2] < 0) { w[2] = -w[2]; V[2] = -V[2]; V[5] = -V[5]; V[8] = -V[8]; }
    transpose33(V, Vt);
    const float s = det33(U) * det33(Vt);
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) { stats[TV_S_FAIL] = TV_FAIL_DEGENERATE_H; return 0; }
    const float aux1 = std::sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = std::sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[] = {aux1, aux1, -aux1, -aux1};
    const float x3[] = {aux3, -aux3, aux3, -aux3};
    const float aux_stheta = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    float sU[9];
    for (int i = 0; i < 9; ++i) sU[i] = s * U[i];
    for (int i = 0; i < 4; ++i) {
      float Rp[9] = {ctheta, 0.f, -stheta[i], 0.f, 1.f, 0.f, stheta[i], 0.f, ctheta};
      mul33(sU, Rp, tmp);
      mul33(tmp, Vt, Rs[i]);
      float tp[3] = {x1[i], 0.f, -x3[i]};
      for (int k = 0; k < 3; ++k) tp[k] *= d1 - d3;
      float tt[3];
      for (int k = 0; k < 3; ++k) tt[k] = U[k * 3] * tp[0] + U[k * 3 + 1] * tp[1] + U[k * 3 + 2] * tp[2];
      const float n = std::sqrt(tt[0] * tt[0] + tt[1] * tt[1] + tt[2] * tt[2]);
      for (int k = 0; k < 3; ++k) ts[i][k] = tt[k] / n;
    }
    const float aux_sphi = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
    for (int i = 0; i < 4; ++i) {
      float Rp[9] = {cphi, 0.f, sphi[i], 0.f, -1.f, 0.f, sphi[i], 0.f, -cphi};
      mul33(sU, Rp, tmp);
      mul33(tmp, Vt, Rs[4 + i]);
      float tp[3] = {x1[i], 0.f, x3[i]};
      for (int k = 0; k < 3; ++k) tp[k] *= d1 + d3;
      float tt[3];
      for (int k = 0; k < 3; ++k) tt[k] = U[k * 3] * tp[0] + U[k * 3 + 1] * tp[1] + U[k * 3 + 2] * tp[2];
      const float n = std::sqrt(tt[0] * tt[0] + tt[1] * tt[1] + tt[2] * tt[2]);
      for (int k = 0; k < 3; ++k) ts[4 + i][k] = tt[k] / n;
    }
    stats[TV_S_NHYP] = 8;
    int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
    float bestParallax = -1;
    for (int i = 0; i < 8; ++i) {
      nGood[i] = S.checkRT(Rs[i], ts[i], bestH, vP3D[i], th2, vGood[i], parallax[i]);
      stats[TV_S_NGOOD0 + i] = nGood[i];
      fstats[TV_F_PARALLAX0 + i] = parallax[i];
      if (nGood[i] > bestGood) {
        secondBestGood = bestGood;
        bestGood = nGood[i];
        bestSolutionIdx = i;
        bestParallax = parallax[i];
      } else if (nGood[i] > secondBestGood) {
        secondBestGood = nGood[i];
      }
    }
    const bool counts = secondBestGood < 0.75 * bestGood && bestGood > minTriangulated && bestGood > 0.9 * Nin;
    if (counts && bestParallax >= minParallax) chosen = bestSolutionIdx;
    else stats[TV_S_FAIL] = counts ? TV_FAIL_PARALLAX : TV_FAIL_AMBIGUOUS;
  } else {   // ReconstructF (:473-560)
    stats[TV_S_MODEL] = 2;
    int Nin = 0;
    for (int i = 0; i < N; ++i) Nin += bestF[i];
    stats[TV_S_NINLIERS] = Nin;
    float Kt[9], tmp[9], E[9], U[9], V[9], Vt[9], w[3];
    transpose33(S.K, Kt);
    mul33(Kt, F, tmp);
    mul33(tmp, S.K, E);
    // DecomposeE (:882-905)
    svd3(E, U, w, V);
    transpose33(V, Vt);
    float t[3] = {U[2], U[5], U[8]};
    const float tn = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (int k = 0; k < 3; ++k) t[k] = t[k] / tn;
    const float W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float Wt[9], R1[9], R2[9];
    transpose33(W, Wt);
    mul33(U, W, tmp);
    mul33(tmp, Vt, R1);
    if (det33(R1) < 0)
      for (int i = 0; i < 9; ++i) R1[i] = -R1[i];
    mul33(U, Wt, tmp);
    mul33(tmp, Vt, R2);
    if (det33(R2) < 0)
      for (int i = 0; i < 9; ++i) R2[i] = -R2[i];
    for (int i = 0; i < 4; ++i) {
      memcpy(Rs[i], (i & 1) ? R2 : R1, sizeof R1);
      for (int k = 0; k < 3; ++k) ts[i][k] = i < 2 ? t[k] : -t[k];
    }
    stats[TV_S_NHYP] = 4;
    for (int i = 0; i < 4; ++i) {
      nGood[i] = S.checkRT(Rs[i], ts[i], bestF, vP3D[i], th2, vGood[i], parallax[i]);
      stats[TV_S_NGOOD0 + i] = nGood[i];
      fstats[TV_F_PARALLAX0 + i] = parallax[i];
    }
    const int maxGood = std::max(nGood[0], std::max(nGood[1], std::max(nGood[2], nGood[3])));
    const int nMinGood = std::max(static_cast<int>(0.9 * Nin), minTriangulated);
    int nsimilar = 0;
    for (int i = 0; i < 4; ++i)
      if (nGood[i] > 0.7 * maxGood) nsimilar++;
    if (maxGood < nMinGood || nsimilar > 1) { stats[TV_S_FAIL] = TV_FAIL_AMBIGUOUS; return 0; }
    int first = 0;
    while (nGood[first] != maxGood) ++first;   // the if / else-if cascade of :525-557 enters the first equal one only
    if (parallax[first] > minParallax) chosen = first;
    else stats[TV_S_FAIL] = TV_FAIL_PARALLAX;
  }
  if (chosen < 0) return 0;
  stats[TV_S_CHOSEN] = chosen;
  for (int i = 0; i < 9; ++i) T21[i] = Rs[chosen][i];
  for (int k = 0; k < 3; ++k) T21[9 + k] = ts[chosen][k];
  for (int i = 0; i < n1; ++i) {
    tri[i] = vGood[chosen][i];
    for (int k = 0; k < 3; ++k) P3D[i * 3 + k] = vP3D[chosen][(size_t)i * 3 + k];
  }
  return 1;
}

}  // extern "C"
