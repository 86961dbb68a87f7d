// CPU oracle of Sim3Solver (reference src/Sim3Solver.cc): an independent restatement of the class with plain arrays for Eigen's
// fixed-size types, built by tests/sim3_solver_oracle.py with g++ -O2 -ffp-contract=off and loaded with ctypes.  Host libm
// throughout (atan2f / sinf / cosf / sqrtf in float, atan2 / log / pow in double), as the reference calls it.
// Conventions it shares with the kernel only through DESIGN.md section 6: Eigen's fixed-size sums taken left to right (coefficient
// order of the expression), Eigen::EigenSolver<Matrix4f> replaced by an FP64 cyclic Jacobi of the symmetric N (fixed sweep order,
// stop when the off-diagonal square sum is <= 1e-30 of the Frobenius square, at most 16 sweeps; the first largest float eigenvalue;
// its eigenvector normalised in double and rounded to float).
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace {

struct V3 { float v[3]; };
struct V2 { float v[2]; };
struct M3 { float m[3][3]; };

struct Camera {
  bool kb8;
  float p[8];
  V2 project(const V3& x) const {   // Pinhole::project / KannalaBrandt8::project (Eigen::Vector3f)
    V2 r;
    const float* v = x.v;
    if (!kb8) {
      r.v[0] = p[0] * v[0] / v[2] + p[2];
      r.v[1] = p[1] * v[1] / v[2] + p[3];
      return r;
    }
    const float x2_plus_y2 = v[0] * v[0] + v[1] * v[1];
    const float theta = atan2f(sqrtf(x2_plus_y2), v[2]);
    const float psi = atan2f(v[1], v[0]);
    const float theta2 = theta * theta;
    const float theta3 = theta * theta2;
    const float theta5 = theta3 * theta2;
    const float theta7 = theta5 * theta2;
    const float theta9 = theta7 * theta2;
    const float rr = theta + p[4] * theta3 + p[5] * theta5 + p[6] * theta7 + p[7] * theta9;
    r.v[0] = p[0] * rr * cosf(psi) + p[2];
    r.v[1] = p[1] * rr * sinf(psi) + p[3];
    return r;
  }
};

V3 affine(const M3& R, const V3& t, const V3& x) {
  V3 o;
  for (int r = 0; r < 3; ++r) o.v[r] = R.m[r][0] * x.v[0] + R.m[r][1] * x.v[1] + R.m[r][2] * x.v[2] + t.v[r];
  return o;
}

int random_int(int mn, int mx, const int*& rnd) {   // DUtils::Random::RandomInt over the recorded rand() sequence
  const int d = mx - mn + 1;
  const int r = *rnd++;
  return int(((double)r / ((double)RAND_MAX + 1.0)) * d) + mn;
}

void jacobi4(double a[4][4], double v[4][4]) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  double fro2 = 0;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) fro2 += a[i][j] * a[i][j];
  static const int PQ[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
  for (int sweep = 0; sweep < 16; ++sweep) {
    double off = 0;
    for (auto& pq : PQ) off += a[pq[0]][pq[1]] * a[pq[0]][pq[1]];
    if (off <= 1e-30 * fro2) break;
    for (auto& pq : PQ) {
      const int p = pq[0], q = pq[1];
      const double apq = a[p][q];
      if (apq == 0.0) continue;
      const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
      const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
      const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
      for (int k = 0; k < 4; ++k) {
        const double akp = a[k][p], akq = a[k][q];
        a[k][p] = c * akp - s * akq;
        a[k][q] = s * akp + c * akq;
      }
      for (int k = 0; k < 4; ++k) {
        const double apk = a[p][k], aqk = a[q][k];
        a[p][k] = c * apk - s * aqk;
        a[q][k] = s * apk + c * aqk;
      }
      a[p][q] = a[q][p] = 0.0;
      for (int k = 0; k < 4; ++k) {
        const double vkp = v[k][p], vkq = v[k][q];
        v[k][p] = c * vkp - s * vkq;
        v[k][q] = s * vkp + c * vkq;
      }
    }
  }
}

struct Solver {
  Camera cam1, cam2;
  bool fixScale;
  int mN1 = 0, N = 0;
  std::vector<V3> X3Dc1, X3Dc2;
  std::vector<V2> P1im1, P2im2;
  std::vector<size_t> maxError1, maxError2;
  std::vector<int> indices1;
  std::vector<size_t> allIndices;
  double ransacProb = 0;
  int minInliers = 0, maxIts = 0, nIterations = 0;
  // current hypothesis
  M3 R12i; V3 t12i; float s12i; float T12i[4][4], T21i[4][4];
  std::vector<bool> inliersi;
  int nInliersi = 0;
  // best
  int bestInliers = 0;
  float bestT12[4][4] = {}, bestR[3][3] = {}, bestt[3] = {}, bestScale = 0;

  void setRansacParameters(double probability, int minIn, int maxIterations) {
    ransacProb = probability;
    minInliers = minIn;
    maxIts = maxIterations;
    N = (int)X3Dc1.size();
    inliersi.resize(N);
    float epsilon = (float)minInliers / N;
    int nIt;
    if (minInliers == N) nIt = 1;
    else nIt = ceil(log(1 - ransacProb) / log(1 - pow(epsilon, 3)));   // as the reference writes it: pow(float, int) is the double pow
    maxIts = std::max(1, std::min(nIt, maxIts));
    nIterations = 0;
  }

  void computeSim3(const float P1[3][3], const float P2[3][3]) {
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
    for (int r = 0; r < 3; ++r) {
      O1[r] = (P1[r][0] + P1[r][1] + P1[r][2]) / 3.0f;
      O2[r] = (P2[r][0] + P2[r][1] + P2[r][2]) / 3.0f;
      for (int c = 0; c < 3; ++c) {
        Pr1[r][c] = P1[r][c] - O1[r];
        Pr2[r][c] = P2[r][c] - O2[r];
      }
    }
    float M[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) M[i][j] = Pr2[i][0] * Pr1[j][0] + Pr2[i][1] * Pr1[j][1] + Pr2[i][2] * Pr1[j][2];
    double N11, N12, N13, N14, N22, N23, N24, N33, N34, N44;
    N11 = M[0][0] + M[1][1] + M[2][2];
    N12 = M[1][2] - M[2][1];
    N13 = M[2][0] - M[0][2];
    N14 = M[0][1] - M[1][0];
    N22 = M[0][0] - M[1][1] - M[2][2];
    N23 = M[0][1] + M[1][0];
    N24 = M[2][0] + M[0][2];
    N33 = -M[0][0] + M[1][1] - M[2][2];
    N34 = M[1][2] + M[2][1];
    N44 = -M[0][0] - M[1][1] + M[2][2];
    const float Nf[4][4] = {{(float)N11, (float)N12, (float)N13, (float)N14},
                            {(float)N12, (float)N22, (float)N23, (float)N24},
                            {(float)N13, (float)N23, (float)N33, (float)N34},
                            {(float)N14, (float)N24, (float)N34, (float)N44}};
    double a[4][4], V[4][4];
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) a[i][j] = Nf[i][j];
    jacobi4(a, V);
    float eval[4];
    for (int k = 0; k < 4; ++k) eval[k] = (float)a[k][k];
    int maxIndex = 0;
    for (int k = 1; k < 4; ++k)
      if (eval[k] > eval[maxIndex]) maxIndex = k;
    double nrm = 0;
    for (int r = 0; r < 4; ++r) nrm += V[r][maxIndex] * V[r][maxIndex];
    nrm = std::sqrt(nrm);
    float evec[4];
    for (int r = 0; r < 4; ++r) evec[r] = (float)(V[r][maxIndex] / nrm);
    float vec[3] = {evec[1], evec[2], evec[3]};
    const float vnorm = sqrtf(vec[0] * vec[0] + vec[1] * vec[1] + vec[2] * vec[2]);
    double ang = atan2(vnorm, evec[0]);
    const float fac = (float)(2 * ang);
    for (float& x : vec) x = fac * x / vnorm;
    // Sophus::SO3f::exp
    const float theta_sq = vec[0] * vec[0] + vec[1] * vec[1] + vec[2] * vec[2];
    float imag, real;
    const float eps = 1e-5f;
    if (theta_sq < eps * eps) {
      const float theta_po4 = theta_sq * theta_sq;
      imag = float(0.5) - float(1.0 / 48.0) * theta_sq + float(1.0 / 3840.0) * theta_po4;
      real = float(1) - float(1.0 / 8.0) * theta_sq + float(1.0 / 384.0) * theta_po4;
    } else {
      const float theta = sqrtf(theta_sq);
      const float half_theta = float(0.5) * theta;
      imag = sinf(half_theta) / theta;
      real = cosf(half_theta);
    }
    const float w = real, x = imag * vec[0], y = imag * vec[1], z = imag * vec[2];
    const float tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    float (&R)[3][3] = R12i.m;
    R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
    float P3[3][3];
    for (int i = 0; i < 3; ++i)
      for (int c = 0; c < 3; ++c) P3[i][c] = R[i][0] * Pr2[0][c] + R[i][1] * Pr2[1][c] + R[i][2] * Pr2[2][c];
    if (!fixScale) {
      float nomf = 0, denf = 0;
      bool first = true;
      for (int c = 0; c < 3; ++c)   // column-major storage order
        for (int r = 0; r < 3; ++r) {
          if (first) { nomf = Pr1[r][c] * P3[r][c]; denf = P3[r][c] * P3[r][c]; first = false; }
          else { nomf += Pr1[r][c] * P3[r][c]; denf += P3[r][c] * P3[r][c]; }
        }
      double nom = nomf, den = denf;
      s12i = nom / den;
    } else {
      s12i = 1.0f;
    }
    float sR[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) sR[i][j] = s12i * R[i][j];
    for (int i = 0; i < 3; ++i) t12i.v[i] = O1[i] - (sR[i][0] * O2[0] + sR[i][1] * O2[1] + sR[i][2] * O2[2]);
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) T12i[i][j] = T21i[i][j] = i == j ? 1.f : 0.f;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) T12i[i][j] = sR[i][j];
      T12i[i][3] = t12i.v[i];
    }
    const float inv = (float)(1.0 / s12i);
    float sRinv[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) sRinv[i][j] = inv * R[j][i];
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) T21i[i][j] = sRinv[i][j];
      float n0 = -sRinv[i][0], n1 = -sRinv[i][1], n2 = -sRinv[i][2];
      T21i[i][3] = n0 * t12i.v[0] + n1 * t12i.v[1] + n2 * t12i.v[2];
    }
  }

  void project(const std::vector<V3>& X, std::vector<V2>& out, const float T[4][4], const Camera& cam) const {
    M3 R;
    V3 t;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) R.m[i][j] = T[i][j];
      t.v[i] = T[i][3];
    }
    out.clear();
    for (const V3& x : X) out.push_back(cam.project(affine(R, t, x)));
  }

  void checkInliers() {
    std::vector<V2> P1im2, P2im1;
    project(X3Dc2, P2im1, T12i, cam1);
    project(X3Dc1, P1im2, T21i, cam2);
    nInliersi = 0;
    for (size_t i = 0; i < P1im1.size(); ++i) {
      const float d10 = P1im1[i].v[0] - P2im1[i].v[0], d11 = P1im1[i].v[1] - P2im1[i].v[1];
      const float d20 = P1im2[i].v[0] - P2im2[i].v[0], d21 = P1im2[i].v[1] - P2im2[i].v[1];
      const float err1 = d10 * d10 + d11 * d11;
      const float err2 = d20 * d20 + d21 * d21;
      if (err1 < maxError1[i] && err2 < maxError2[i]) {
        inliersi[i] = true;
        nInliersi++;
      } else {
        inliersi[i] = false;
      }
    }
  }

  // iterate(nIt, bNoMore, vbInliers, nInliers, bConverge); returns whether bestSim3 was assigned
  void iterate(int nIt, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge, bool& assigned, float out[4][4],
               const int*& rnd, int* hyp, int hypCap) {
    bNoMore = false;
    bConverge = false;
    assigned = false;
    vbInliers.assign(mN1, false);
    nInliers = 0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) out[i][j] = i == j ? 1.f : 0.f;
    if (N < minInliers || N < 3) {
      bNoMore = true;
      return;
    }
    int nCurrent = 0;
    while (nIterations < maxIts && nCurrent < nIt) {
      nCurrent++;
      const int g = nIterations;
      nIterations++;
      std::vector<size_t> avail = allIndices;
      float P1[3][3], P2[3][3];
      for (short i = 0; i < 3; ++i) {
        int randi = random_int(0, (int)(avail.size() - 1), rnd);
        int idx = (int)avail[randi];
        for (int r = 0; r < 3; ++r) {
          P1[r][i] = X3Dc1[idx].v[r];
          P2[r][i] = X3Dc2[idx].v[r];
        }
        avail[randi] = avail.back();
        avail.pop_back();
      }
      computeSim3(P1, P2);
      checkInliers();
      if (hyp && g < hypCap) hyp[g] = nInliersi;
      if (nInliersi >= bestInliers) {
        bestInliers = nInliersi;
        for (int i = 0; i < 4; ++i)
          for (int j = 0; j < 4; ++j) bestT12[i][j] = T12i[i][j];
        for (int i = 0; i < 3; ++i) {
          for (int j = 0; j < 3; ++j) bestR[i][j] = R12i.m[i][j];
          bestt[i] = t12i.v[i];
        }
        bestScale = s12i;
        for (int i = 0; i < 4; ++i)
          for (int j = 0; j < 4; ++j) out[i][j] = bestT12[i][j];
        assigned = true;
        if (nInliersi > minInliers) {
          nInliers = nInliersi;
          for (int i = 0; i < N; ++i)
            if (inliersi[i]) vbInliers[indices1[i]] = true;
          bConverge = true;
          return;
        }
      }
    }
    if (nIterations >= maxIts) bNoMore = true;
  }
};

}  // namespace

extern "C" {

// One problem: the constructor + SetRansacParameters, then nCalls calls of iterate(callIts[k], ...) that continue one another
// (a call is skipped once an earlier one converged or reported bNoMore, as LoopClosing's loop does).  rnd holds the rand() values in
// draw order; hyp [hypCap] receives the per-iteration inlier counts (pre-filled by the caller).  Per call k: res[k][8] = converged,
// noMore, nInliers, iterations after the call, bestInliers, assigned (bestSim3 set in this call), N, budget; sim3[k][16] the return
// value of the bConverge overload (identity where the reference leaves it uninitialised); mask[k][n].  best[29] after the last call
// made: mBestT12 (16), mBestRotation (9), mBestTranslation (3), mBestScale.  Returns the number of calls made.
int sim3s_oracle_run(int n, const uint8_t* entry, const float* Xw1, const float* Xw2, const float* s2_1, const float* s2_2, const float* T1w,
                     const float* T2w, const float* cam1, const float* cam2, int fixScale, double probability, int minInliers,
                     int maxIterations, int nCalls, const int* callIts, const int* rnd, int* hyp, int hypCap, int* res, float* sim3,
                     uint8_t* mask, float* best) {
  Solver S;
  S.cam1.kb8 = cam1[0] != 0.f;
  S.cam2.kb8 = cam2[0] != 0.f;
  for (int i = 0; i < 8; ++i) { S.cam1.p[i] = cam1[1 + i]; S.cam2.p[i] = cam2[1 + i]; }
  S.fixScale = fixScale != 0;
  S.mN1 = n;
  M3 R1, R2;
  V3 t1, t2;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) { R1.m[r][c] = T1w[r * 3 + c]; R2.m[r][c] = T2w[r * 3 + c]; }
    t1.v[r] = T1w[9 + r];
    t2.v[r] = T2w[9 + r];
  }
  size_t idx = 0;
  for (int i1 = 0; i1 < n; ++i1) {
    const uint8_t e = entry[i1];
    if (!(e & 1)) continue;                 // vpMatched12[i1]
    if (!(e & 2)) continue;                 // pMP1
    if ((e & 4) || (e & 8)) continue;       // isBad
    if ((e & 16) || (e & 32)) continue;     // indexKF1 < 0 || indexKF2 < 0
    S.maxError1.push_back(9.210 * s2_1[i1]);
    S.maxError2.push_back(9.210 * s2_2[i1]);
    S.indices1.push_back(i1);
    V3 a, b;
    for (int r = 0; r < 3; ++r) { a.v[r] = Xw1[i1 * 3 + r]; b.v[r] = Xw2[i1 * 3 + r]; }
    S.X3Dc1.push_back(affine(R1, t1, a));
    S.X3Dc2.push_back(affine(R2, t2, b));
    S.allIndices.push_back(idx);
    idx++;
  }
  for (const V3& x : S.X3Dc1) S.P1im1.push_back(S.cam1.project(x));
  for (const V3& x : S.X3Dc2) S.P2im2.push_back(S.cam2.project(x));
  S.setRansacParameters(probability, minInliers, maxIterations);
  const int* rp = rnd;
  int made = 0;
  for (int k = 0; k < nCalls; ++k) {
    bool noMore, conv, assigned;
    std::vector<bool> vb;
    int nIn;
    float out[4][4];
    S.iterate(callIts[k], noMore, vb, nIn, conv, assigned, out, rp, hyp, hypCap);
    int* rr = res + 8 * k;
    rr[0] = conv; rr[1] = noMore; rr[2] = nIn; rr[3] = S.nIterations; rr[4] = S.bestInliers; rr[5] = assigned; rr[6] = S.N;
    rr[7] = S.maxIts;
    for (int i = 0; i < 16; ++i) sim3[16 * k + i] = out[i / 4][i % 4];
    for (int i = 0; i < n; ++i) mask[(size_t)n * k + i] = vb[i] ? 1 : 0;
    made++;
    if (conv || noMore) break;
  }
  for (int i = 0; i < 16; ++i) best[i] = S.bestT12[i / 4][i % 4];
  for (int i = 0; i < 9; ++i) best[16 + i] = S.bestR[i / 3][i % 3];
  for (int i = 0; i < 3; ++i) best[25 + i] = S.bestt[i];
  best[28] = S.bestScale;
  return made;
}

// SetRansacParameters' budget as the reference computes it, for the exhaustive CPU check of the kernel's formula.
int sim3s_oracle_budget(int N, int minInliers, double probability, int maxIterations) {
  float epsilon = (float)minInliers / N;
  int nIt;
  if (minInliers == N) nIt = 1;
  else {
    volatile double v = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
    nIt = (int)v;   // x86-64: cvttsd2si, INT_MIN for NaN and out-of-range values
  }
  return std::max(1, std::min(nIt, maxIterations));
}

}  // extern "C"
