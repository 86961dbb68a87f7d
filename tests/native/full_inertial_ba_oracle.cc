// TEST INFRASTRUCTURE.  FP64 oracle of Optimizer::FullInertialBA (reference src/Optimizer.cc:364-760) on the flattened graph of
// morb_full_inertial_ba: the edges and the Levenberg-Marquardt loop of merge_inertial_ba_oracle.cc (ImuCamPose vertices, EdgeMono /
// EdgeStereo on either camera of a rig, EdgeInertial, EdgeGyroRW, EdgeAccRW; g2o's LM with ORB-SLAM's stop rule from the user lambda 1e-5,
// one optimize(its)), the shared gyro / accelerometer bias vertices of bInit with EdgePriorGyro / EdgePriorAcc, and global_ba_oracle.cc's
// skyline LDL^T without pivoting in place of the dense one: the envelope is that of the 3 x 3 block rows as csrc/full_inertial_ba.hip lays
// them out, and a skyline only skips exact zeros.  One thread, no dependency but the C++ library.
// -DFIB_ORACLE_DENSE: the factorisation runs over the whole lower triangle, for the test that the skyline skips nothing but exact zeros.
// -DFIB_ORACLE_REVERSE: points and links are visited in reverse order (another summation order), for the test that rounding does not move the
// corpus.  Keyframe kinds: 0 free (15 unknowns; 9 with bInit), 1 / 2 fixed, 3 free in the pose only (6 unknowns; its velocity and bias
// vertices carry no edge, g2o leaves them out of the active set; without a visual edge it is not in the system at all).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

namespace {

// morb_imu_preintegrated (include/morb_hip.h) as 310 floats
struct Preint { float dT, dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], C[225], b[6], nga[6], ngaWalk[6], avgA[3], avgW[3]; };
static_assert(sizeof(Preint) == 310 * 4, "record layout");

void mm(const double* A, const double* B, double* C) {
  double T[9];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) T[r * 3 + c] = A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c] + A[r * 3 + 2] * B[6 + c];
  memcpy(C, T, sizeof T);
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

void exp_so3(const double* w, double* R) {   // G2oTypes.cc:783-796
  const double d2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], d = std::sqrt(d2);
  double W[9], WW[9];
  hat(w, W); mm(W, W, WW);
  if (d < 1e-5) for (int k = 0; k < 9; ++k) R[k] = I3[k] + W[k] + 0.5 * WW[k];
  else { const double s = std::sin(d), c = std::cos(d); for (int k = 0; k < 9; ++k) R[k] = I3[k] + W[k] * s / d + WW[k] * (1.0 - c) / d2; }
}
void log_so3(const double* R, double* w) {   // G2oTypes.cc:798-811 (`0.5f` as there)
  const double trc = R[0] + R[4] + R[8];
  w[0] = (R[7] - R[5]) / 2; w[1] = (R[2] - R[6]) / 2; w[2] = (R[3] - R[1]) / 2;
  const double ct = (trc - 1.0) * 0.5f;
  if (ct > 1 || ct < -1) return;
  const double th = std::acos(ct), s = std::sin(th);
  if (std::fabs(s) < 1e-5) return;
  for (int k = 0; k < 3; ++k) w[k] = th * w[k] / s;
}
void inv_right_jac(const double* v, double* J) {   // G2oTypes.cc:817-829
  const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], d = std::sqrt(d2);
  if (d < 1e-5) { memcpy(J, I3, sizeof I3); return; }
  double W[9], WW[9];
  hat(v, W); mm(W, W, WW);
  const double k2 = 1.0 / d2 - (1.0 + std::cos(d)) / (2.0 * d * std::sin(d));
  for (int k = 0; k < 9; ++k) J[k] = I3[k] + W[k] / 2 + WW[k] * k2;
}
void right_jac(const double* v, double* J) {   // G2oTypes.cc:835-848
  const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], d = std::sqrt(d2);
  if (d < 1e-5) { memcpy(J, I3, sizeof I3); return; }
  double W[9], WW[9];
  hat(v, W); mm(W, W, WW);
  for (int k = 0; k < 9; ++k) J[k] = I3[k] - W[k] * (1.0 - std::cos(d)) / d2 + WW[k] * (d - std::sin(d)) / (d2 * d);
}

// n x n inverse by Gauss-Jordan with partial pivoting
bool invert(const double* A, int n, double* Ainv) {
  std::vector<double> M((size_t)n * 2 * n, 0.0);
  const int w = 2 * n;
  for (int r = 0; r < n; ++r) { for (int c = 0; c < n; ++c) M[(size_t)r * w + c] = A[r * n + c]; M[(size_t)r * w + n + r] = 1.0; }
  for (int c = 0; c < n; ++c) {
    int p = c;
    for (int r = c + 1; r < n; ++r) if (std::fabs(M[(size_t)r * w + c]) > std::fabs(M[(size_t)p * w + c])) p = r;
    if (M[(size_t)p * w + c] == 0.0) return false;
    if (p != c) for (int k = 0; k < w; ++k) std::swap(M[(size_t)p * w + k], M[(size_t)c * w + k]);
    const double inv = 1.0 / M[(size_t)c * w + c];
    for (int k = 0; k < w; ++k) M[(size_t)c * w + k] *= inv;
    for (int r = 0; r < n; ++r) {
      const double f = M[(size_t)r * w + c];
      if (r != c && f != 0.0) for (int k = 0; k < w; ++k) M[(size_t)r * w + k] -= f * M[(size_t)c * w + k];
    }
  }
  for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) Ainv[r * n + c] = M[(size_t)r * w + n + c];
  return true;
}
// A = V diag(e) V^T of a symmetric matrix, cyclic Jacobi
void sym_eig(const double* A, int n, double* e, double* V) {
  std::vector<double> a(A, A + (size_t)n * n);
  for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) V[r * n + c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0, diag = 0;
    for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) (r == c ? diag : off) += a[r * n + c] * a[r * n + c];
    if (off <= 1e-30 * diag) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        if (a[p * n + q] == 0.0) continue;
        const double theta = (a[q * n + q] - a[p * n + p]) / (2.0 * a[p * n + q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) { const double x = a[k * n + p], y = a[k * n + q]; a[k * n + p] = c * x - s * y; a[k * n + q] = s * x + c * y; }
        for (int k = 0; k < n; ++k) { const double x = a[p * n + k], y = a[q * n + k]; a[p * n + k] = c * x - s * y; a[q * n + k] = s * x + c * y; }
        for (int k = 0; k < n; ++k) { const double x = V[k * n + p], y = V[k * n + q]; V[k * n + p] = c * x - s * y; V[k * n + q] = s * x + c * y; }
      }
  }
  for (int k = 0; k < n; ++k) e[k] = a[k * n + k];
}
// EdgeInertial's information (G2oTypes.cc:484-491): C(0:9, 0:9)^-1, symmetrised, eigenvalues below 1e-12 set to zero
void inertial_information(const float* C15, double* Info) {
  double C9[81], Inv[81], S[81], e[9], V[81];
  for (int r = 0; r < 9; ++r) for (int c = 0; c < 9; ++c) C9[r * 9 + c] = (double)C15[r * 15 + c];
  if (!invert(C9, 9, Inv)) { memset(Info, 0, sizeof(double) * 81); return; }
  for (int r = 0; r < 9; ++r) for (int c = 0; c < 9; ++c) S[r * 9 + c] = (Inv[r * 9 + c] + Inv[c * 9 + r]) / 2;
  sym_eig(S, 9, e, V);
  for (int k = 0; k < 9; ++k) if (e[k] < 1e-12) e[k] = 0;
  for (int r = 0; r < 9; ++r)
    for (int c = 0; c < 9; ++c) { double s = 0; for (int k = 0; k < 9; ++k) s += V[r * 9 + k] * e[k] * V[c * 9 + k]; Info[r * 9 + c] = s; }
}
// H = L D L^T without pivoting over a skyline, in place, then the two substitutions: what lies left of a row's first column is zero and
// stays zero, so nothing but exact zeros is skipped.  A zero or NaN pivot is a failed factorisation.
struct Skyline {   // the lower triangle of a symmetric matrix, row r stored from column first[r] to r
  int n = 0;
  std::vector<int> first;
  std::vector<size_t> off;
  std::vector<double> v;
  void shape(const std::vector<int>& f) {
    n = (int)f.size(); first = f; off.assign(n + 1, 0);
    for (int r = 0; r < n; ++r) off[r + 1] = off[r] + (size_t)(r - first[r] + 1);
    v.assign(off[n], 0.0);
  }
  double& at(int r, int c) { return v[off[r] + (size_t)(c - first[r])]; }   // r >= c >= first[r]
};
bool skyline_ldlt_solve(Skyline& A, const double* b, double* x) {   // in place: L below the diagonal, D on it
  const int n = A.n;
  std::vector<double> y(b, b + n);
  for (int i = 0; i < n; ++i)
    for (int j = A.first[i]; j <= i; ++j) {
      double s = A.at(i, j);
      for (int k = std::max(A.first[i], A.first[j]); k < j; ++k) s -= A.at(i, k) * A.at(k, k) * A.at(j, k);
      if (i == j) { if (s == 0 || s != s) return false; A.at(i, i) = s; }
      else A.at(i, j) = s / A.at(j, j);
    }
  for (int r = 0; r < n; ++r) for (int c = A.first[r]; c < r; ++c) y[r] -= A.at(r, c) * y[c];
  for (int k = 0; k < n; ++k) y[k] /= A.at(k, k);
  for (int r = n - 1; r >= 0; --r) {
    x[r] = y[r];
    for (int c = A.first[r]; c < r; ++c) y[c] -= A.at(r, c) * y[r];
  }
  return true;
}

// the cameras behind a body pose: one pinhole (fx fy cx cy bf), or the KannalaBrandt8 rig (rig28: left 8, right 8, Rrl 9, trl 3)
struct Rig {
  bool kb8 = false;
  float pin[5] = {0, 0, 0, 0, 0};
  float kb[2][8];
  double Rcb[2][9], tcb[2][3], Rbc[2][9], tbc[2][3];
  void set(const float* Tbc12, const float* cam5, const float* rig28) {
    double Rbc0[9], tbc0[3];
    for (int k = 0; k < 9; ++k) Rbc0[k] = Tbc12[k];
    for (int k = 0; k < 3; ++k) tbc0[k] = Tbc12[9 + k];
    memcpy(Rbc[0], Rbc0, sizeof Rbc0); memcpy(tbc[0], tbc0, sizeof tbc0);
    tr(Rbc0, Rcb[0]); mv(Rcb[0], tbc0, tcb[0]);
    for (double& c : tcb[0]) c = -c;
    memcpy(Rcb[1], Rcb[0], sizeof Rcb[0]); memcpy(tcb[1], tcb[0], sizeof tcb[0]); memcpy(Rbc[1], Rbc[0], sizeof Rbc[0]); memcpy(tbc[1], tbc[0], sizeof tbc[0]);
    if (cam5) memcpy(pin, cam5, sizeof pin);
    if (!rig28) return;
    kb8 = true;   // G2oTypes.cc:104-113
    memcpy(kb[0], rig28, 32); memcpy(kb[1], rig28 + 8, 32);
    double Rrl[9], trl[3];
    for (int k = 0; k < 9; ++k) Rrl[k] = rig28[16 + k];
    for (int k = 0; k < 3; ++k) trl[k] = rig28[25 + k];
    mm(Rrl, Rcb[0], Rcb[1]); mv(Rrl, tcb[0], tcb[1]);
    for (int k = 0; k < 3; ++k) tcb[1][k] += trl[k];
    tr(Rcb[1], Rbc[1]); mv(Rbc[1], tcb[1], tbc[1]);
    for (double& c : tbc[1]) c = -c;
  }
};
struct KF {
  double Rwb[9], twb[3], v[3], bg[3], ba[3];
  double Rcw[2][9], tcw[2][3];
  int off = -1, wid = 0;
  void refresh(const Rig& g) {   // G2oTypes.cc:209-215
    double Rbw[9], tbw[3];
    tr(Rwb, Rbw); mv(Rbw, twb, tbw);
    for (double& c : tbw) c = -c;
    for (int cam = 0; cam < (g.kb8 ? 2 : 1); ++cam) {
      mm(g.Rcb[cam], Rbw, Rcw[cam]); mv(g.Rcb[cam], tbw, tcw[cam]);
      for (int k = 0; k < 3; ++k) tcw[cam][k] += g.tcb[cam][k];
    }
  }
  void load(const Rig& g, const double* s) {
    memcpy(Rwb, s, 72); memcpy(twb, s + 9, 24); memcpy(v, s + 12, 24); memcpy(bg, s + 15, 24); memcpy(ba, s + 18, 24);
    refresh(g);
  }
  void store(double* s) const { memcpy(s, Rwb, 72); memcpy(s + 9, twb, 24); memcpy(s + 12, v, 24); memcpy(s + 15, bg, 24); memcpy(s + 18, ba, 24); }
  // ImuCamPose::Update (G2oTypes.cc:192-216; its NormalizeRotation result is discarded there) and the additive vertices; n = 15 or 6
  void oplus(const Rig& g, const double* dx, int n) {
    double t[3], dR[9];
    mv(Rwb, dx + 3, t);
    for (int k = 0; k < 3; ++k) twb[k] += t[k];
    exp_so3(dx, dR); mm(Rwb, dR, Rwb);
    refresh(g);
    if (n >= 9) for (int k = 0; k < 3; ++k) v[k] += dx[6 + k];
    if (n == 15) for (int k = 0; k < 3; ++k) { bg[k] += dx[9 + k]; ba[k] += dx[12 + k]; }
  }
};

// projection of a camera-frame point and its 2 x 3 Jacobian (Pinhole.cpp:38-44, :76-86; KannalaBrandt8.cpp project(Vector3d) with atan2f / sqrtf
// on doubles as there, projectJac)
void project(const Rig& g, int cam, const double* x, double* uv) {
  if (g.kb8) {
    const float* p = g.kb[cam];
    const double r2 = x[0] * x[0] + x[1] * x[1];
    const double th = atan2f(sqrtf((float)r2), (float)x[2]), psi = atan2f((float)x[1], (float)x[0]);
    const double t2 = th * th, t3 = th * t2, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
    const double r = th + p[4] * t3 + p[5] * t5 + p[6] * t7 + p[7] * t9;
    uv[0] = p[0] * r * std::cos(psi) + p[2]; uv[1] = p[1] * r * std::sin(psi) + p[3];
    return;
  }
  uv[0] = g.pin[0] * x[0] / x[2] + g.pin[2]; uv[1] = g.pin[1] * x[1] / x[2] + g.pin[3];
}
void project_jac(const Rig& g, int cam, const double* v, double* J) {
  if (g.kb8) {
    const float* p = g.kb[cam];
    const double x2 = v[0] * v[0], y2 = v[1] * v[1], z2 = v[2] * v[2], r2 = x2 + y2, r = std::sqrt(r2), r3 = r2 * r;
    const double th = std::atan2(r, v[2]), t2 = th * th, t3 = t2 * th, t4 = t2 * t2, t5 = t4 * th, t6 = t2 * t4, t7 = t6 * th, t8 = t4 * t4, t9 = t8 * th;
    const double f = th + t3 * p[4] + t5 * p[5] + t7 * p[6] + t9 * p[7], fd = 1 + 3 * p[4] * t2 + 5 * p[5] * t4 + 7 * p[6] * t6 + 9 * p[7] * t8;
    J[0] = p[0] * (fd * v[2] * x2 / (r2 * (r2 + z2)) + f * y2 / r3);
    J[1] = p[0] * (fd * v[2] * v[1] * v[0] / (r2 * (r2 + z2)) - f * v[1] * v[0] / r3);
    J[2] = -p[0] * fd * v[0] / (r2 + z2);
    J[3] = p[1] * (fd * v[2] * v[1] * v[0] / (r2 * (r2 + z2)) - f * v[1] * v[0] / r3);
    J[4] = p[1] * (fd * v[2] * y2 / (r2 * (r2 + z2)) + f * x2 / r3);
    J[5] = -p[1] * fd * v[1] / (r2 + z2);
    return;
  }
  J[0] = g.pin[0] / v[2]; J[1] = 0; J[2] = -g.pin[0] * v[0] / (v[2] * v[2]);
  J[3] = 0; J[4] = g.pin[1] / v[2]; J[5] = -g.pin[1] * v[1] / (v[2] * v[2]);
}
// EdgeMono / EdgeStereo (G2oTypes.h:336-388, :425-464; G2oTypes.cc:171-186, :334-442): rows, error, d / d pose (rows x 6), d / d point (rows x 3)
int vis_edge(const Rig& g, const KF& K, int cam, const double* X, const float* obs, bool stereo, double* err, double* Jp, double* Jl) {
  const int d = stereo ? 3 : 2;
  double xc[3], uv[2];
  mv(K.Rcw[cam], X, xc);
  for (int k = 0; k < 3; ++k) xc[k] += K.tcw[cam][k];
  project(g, cam, xc, uv);
  err[0] = obs[0] - uv[0]; err[1] = obs[1] - uv[1]; err[2] = 0;
  const double bf = g.pin[4];
  if (stereo) err[2] = obs[2] - (uv[0] - bf * (1 / xc[2]));
  if (!Jp && !Jl) return d;
  double pj[9];
  project_jac(g, cam, xc, pj);
  if (stereo) { pj[6] = pj[0]; pj[7] = pj[1]; pj[8] = pj[2] + bf * (1.0 / (xc[2] * xc[2])); }
  if (Jl)
    for (int r = 0; r < d; ++r) for (int c = 0; c < 3; ++c) Jl[r * 3 + c] = -(pj[r * 3] * K.Rcw[cam][c] + pj[r * 3 + 1] * K.Rcw[cam][3 + c] + pj[r * 3 + 2] * K.Rcw[cam][6 + c]);
  if (Jp) {
    double xb[3], PR[9];
    mv(g.Rbc[cam], xc, xb);
    for (int k = 0; k < 3; ++k) xb[k] += g.tbc[cam][k];
    const double x = xb[0], y = xb[1], z = xb[2];
    const double S[18] = {0.0, z, -y, 1.0, 0.0, 0.0, -z, 0.0, x, 0.0, 1.0, 0.0, y, -x, 0.0, 0.0, 0.0, 1.0};
    for (int r = 0; r < d; ++r) for (int c = 0; c < 3; ++c) PR[r * 3 + c] = pj[r * 3] * g.Rcb[cam][c] + pj[r * 3 + 1] * g.Rcb[cam][3 + c] + pj[r * 3 + 2] * g.Rcb[cam][6 + c];
    for (int r = 0; r < d; ++r) for (int c = 0; c < 6; ++c) Jp[r * 6 + c] = PR[r * 3] * S[c] + PR[r * 3 + 1] * S[6 + c] + PR[r * 3 + 2] * S[12 + c];
  }
  return d;
}

// GetDeltaRotation / Velocity / Position at the bias of keyframe 1 (ImuTypes.cc:289-312), in float as there; NormalizeRotation = the polar factor
void preint_delta(const Preint& P, const float* b1 /* acc, gyro */, double* dR, double* dV, double* dP) {
  const float dbg[3] = {b1[3] - P.b[3], b1[4] - P.b[4], b1[5] - P.b[5]}, dba[3] = {b1[0] - P.b[0], b1[1] - P.b[1], b1[2] - P.b[2]};
  auto mvf = [](const float* A, const float* v, float* o) { for (int r = 0; r < 3; ++r) o[r] = A[r * 3] * v[0] + A[r * 3 + 1] * v[1] + A[r * 3 + 2] * v[2]; };
  float w[3];
  mvf(P.JRg, dbg, w);
  const float t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], t = std::sqrt(t2);
  const float W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  float WW[9], E[9], Rf[9];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) WW[r * 3 + c] = W[r * 3] * W[c] + W[r * 3 + 1] * W[3 + c] + W[r * 3 + 2] * W[6 + c];
  const float If[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (t < 1e-5f) for (int k = 0; k < 9; ++k) E[k] = If[k] + W[k] + 0.5f * WW[k];
  else { const float s = std::sin(t), c = std::cos(t); for (int k = 0; k < 9; ++k) E[k] = If[k] + W[k] * s / t + WW[k] * (1.0f - c) / t2; }
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rf[r * 3 + c] = P.dR[r * 3] * E[c] + P.dR[r * 3 + 1] * E[3 + c] + P.dR[r * 3 + 2] * E[6 + c];
  double X[9];
  for (int k = 0; k < 9; ++k) X[k] = Rf[k];
  for (int it = 0; it < 6; ++it) {   // X <- (X + X^-T) / 2
    const double c00 = X[4] * X[8] - X[5] * X[7], c01 = X[5] * X[6] - X[3] * X[8], c02 = X[3] * X[7] - X[4] * X[6];
    const double inv = 1.0 / (X[0] * c00 + X[1] * c01 + X[2] * c02);
    const double Cf[9] = {c00, c01, c02, X[2] * X[7] - X[1] * X[8], X[0] * X[8] - X[2] * X[6], X[1] * X[6] - X[0] * X[7],
                          X[1] * X[5] - X[2] * X[4], X[2] * X[3] - X[0] * X[5], X[0] * X[4] - X[1] * X[3]};
    for (int k = 0; k < 9; ++k) X[k] = 0.5 * (X[k] + Cf[k] * inv);
  }
  for (int k = 0; k < 9; ++k) dR[k] = (float)X[k];
  float g1[3], a1[3];
  mvf(P.JVg, dbg, g1); mvf(P.JVa, dba, a1);
  for (int k = 0; k < 3; ++k) dV[k] = P.dV[k] + g1[k] + a1[k];
  mvf(P.JPg, dbg, g1); mvf(P.JPa, dba, a1);
  for (int k = 0; k < 3; ++k) dP[k] = P.dP[k] + g1[k] + a1[k];
}
// EdgeInertial::computeError / linearizeOplus (G2oTypes.cc:493-585).  J: 9 x 24, columns = pose1 (rotation, translation), v1, bg1, ba1, pose2, v2
void inertial_edge(const Preint& P, const KF& K1, const KF& K2, double* err, double* J) {
  const float b1[6] = {(float)K1.ba[0], (float)K1.ba[1], (float)K1.ba[2], (float)K1.bg[0], (float)K1.bg[1], (float)K1.bg[2]};
  double dR[9], dV[3], dP[3];
  preint_delta(P, b1, dR, dV, dP);
  const double dt = P.dT, g[3] = {0, 0, -(double)9.81f};
  double Rbw1[9], dRt[9], M[9], eR[9], er[3], t1[3], t2[3], a1[3], a2[3];
  tr(K1.Rwb, Rbw1); tr(dR, dRt); mm(dRt, Rbw1, M); mm(M, K2.Rwb, eR);
  log_so3(eR, er);
  for (int k = 0; k < 3; ++k) { t1[k] = K2.v[k] - K1.v[k] - g[k] * dt; t2[k] = K2.twb[k] - K1.twb[k] - K1.v[k] * dt - g[k] * dt * dt / 2; }
  mv(Rbw1, t1, a1); mv(Rbw1, t2, a2);
  for (int k = 0; k < 3; ++k) { err[k] = er[k]; err[3 + k] = a1[k] - dV[k]; err[6 + k] = a2[k] - dP[k]; }
  if (!J) return;
  memset(J, 0, sizeof(double) * 216);
  auto put = [&](int r0, int c0, const double* B, double sgn) { for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) J[(r0 + r) * 24 + c0 + c] = sgn * B[r * 3 + c]; };
  double invJr[9], Rbw2[9], T[9], T2[9], W[9], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9];
  for (int k = 0; k < 9; ++k) { JRg[k] = P.JRg[k]; JVg[k] = P.JVg[k]; JVa[k] = P.JVa[k]; JPg[k] = P.JPg[k]; JPa[k] = P.JPa[k]; }
  inv_right_jac(er, invJr);
  tr(K2.Rwb, Rbw2);
  mm(invJr, Rbw2, T); mm(T, K1.Rwb, T2);
  put(0, 0, T2, -1.0);                       // d er / d phi1
  hat(a1, W); put(3, 0, W, 1.0);             // d ev / d phi1
  {
    double t3[3], a3[3];
    for (int k = 0; k < 3; ++k) t3[k] = K2.twb[k] - K1.twb[k] - K1.v[k] * dt - 0.5 * g[k] * dt * dt;
    mv(Rbw1, t3, a3);
    hat(a3, W); put(6, 0, W, 1.0);           // d ep / d phi1
  }
  put(6, 3, I3, -1.0);                       // d ep / d t1 (body frame)
  put(3, 6, Rbw1, -1.0);                     // d ev / d v1
  { double B[9]; for (int k = 0; k < 9; ++k) B[k] = Rbw1[k] * dt; put(6, 6, B, -1.0); }
  {
    const float dbgf[3] = {b1[3] - P.b[3], b1[4] - P.b[4], b1[5] - P.b[5]};
    const double dbg[3] = {dbgf[0], dbgf[1], dbgf[2]};
    double w3[3], rj[9], eRt[9];
    mv(JRg, dbg, w3); right_jac(w3, rj); tr(eR, eRt);
    mm(invJr, eRt, T); mm(T, rj, T2); mm(T2, JRg, T);
    put(0, 9, T, -1.0); put(3, 9, JVg, -1.0); put(6, 9, JPg, -1.0);
  }
  put(3, 12, JVa, -1.0); put(6, 12, JPa, -1.0);
  put(0, 15, invJr, 1.0);
  mm(Rbw1, K2.Rwb, T); put(6, 18, T, 1.0);
  put(3, 21, Rbw1, 1.0);
}

double huber(double delta, double e2, double* w) {   // robust_kernel_impl.cpp:65-91: rho(e2), rho'(e2)
  const double d2 = delta * delta;
  if (e2 <= d2) { *w = 1.0; return e2; }
  const double s = std::sqrt(e2);
  *w = delta / s;
  return 2 * s * delta - d2;
}

// The whole problem and the pieces of one LM iteration on it; run() and gradient() below drive them.
struct Problem {
  int nKF, nMP, nE, nI, bInit;
  const int *eKF, *eMP, *iKF1, *iKF2;
  const float *eObs, *eInv;
  const uint8_t* eRight;
  bool rig;
  Rig g;
  double priorG, priorA;
  std::vector<KF> S;
  std::vector<double> pts;
  double sb[6];   // the shared biases: gyro, accelerometer
  std::vector<Preint> pre;
  int P = 0, offB = -1, nBlocks = 0;
  std::vector<int> firstScalar;   // the skyline: every scalar row of a 3 x 3 block row begins at the block row's first column
  std::vector<int> ptOrder, linkOrder;
  std::vector<std::vector<int>> byPoint;
  std::vector<double> InfoI, InfoG, InfoA, vErr, iErr, gErr, aErr;
  Skyline H;
  std::vector<double> b, Hll, Hpl, x;
  double thMono, thStereo, thInertial;

  bool stereo(int e) const { return !rig && !(eObs[3 * e + 2] < 0); }
  int camOf(int e) const { return rig && eRight && eRight[e] ? 1 : 0; }
  static double quad(const double* e, const double* Om, int n) { double s = 0; for (int r = 0; r < n; ++r) for (int c = 0; c < n; ++c) s += e[r] * Om[r * n + c] * e[c]; return s; }
  double visChi2(int e) const { const double info = eInv[e]; double s = 0; for (int k = 0; k < (stereo(e) ? 3 : 2); ++k) s += vErr[3 * e + k] * info * vErr[3 * e + k]; return s; }
  KF link_kf1(int i) const {   // keyframe 1 of a link at the biases its EdgeInertial hangs on
    KF K = S[iKF1[i]];
    if (bInit) for (int k = 0; k < 3; ++k) { K.bg[k] = sb[k]; K.ba[k] = sb[3 + k]; }
    return K;
  }

  void setup(int nKF_, const float* kfState21, const uint8_t* kfKind, int nMP_, const float* mpPos, int nE_, const int* eKF_, const int* eMP_,
             const float* eObs_, const uint8_t* eRight_, const float* eInv_, int nI_, const int* iKF1_, const int* iKF2_, const float* iPre310,
             const float* cam5, const float* rig28, const float* Tbc12, int bInit_, double priorG_, double priorA_, const float* bias6) {
    nKF = nKF_; nMP = nMP_; nE = nE_; nI = nI_; bInit = bInit_ ? 1 : 0; eKF = eKF_; eMP = eMP_; eObs = eObs_; eRight = eRight_; eInv = eInv_;
    iKF1 = iKF1_; iKF2 = iKF2_; rig = rig28 != nullptr; priorG = priorG_; priorA = priorA_;
    g.set(Tbc12, cam5, rig28);
    thMono = (double)(float)std::sqrt(5.991); thStereo = (double)(float)std::sqrt(7.815); thInertial = std::sqrt(16.92);
    std::vector<char> seen(nKF, 0);
    for (int e = 0; e < nE; ++e) seen[eKF[e]] = 1;
    S.resize(nKF);
    std::vector<int> sys;
    for (int k = 0; k < nKF; ++k) {
      double s[21];
      for (int i = 0; i < 21; ++i) s[i] = kfState21[21 * k + i];
      S[k].load(g, s);
      S[k].wid = kfKind[k] == 0 ? (bInit ? 9 : 15) : (kfKind[k] == 3 && seen[k]) ? 6 : 0;
      if (S[k].wid) { S[k].off = P; P += S[k].wid; sys.push_back(k); }
    }
    for (int k = 0; k < 6; ++k) sb[k] = bInit ? (double)bias6[k] : 0.0;
    if (bInit && P) { offB = P; P += 6; }
    pts.assign(mpPos, mpPos + (size_t)3 * nMP);
    pre.resize(nI);
    if (nI) memcpy(pre.data(), iPre310, sizeof(Preint) * nI);
    ptOrder.resize(nMP); linkOrder.resize(nI);
    for (int l = 0; l < nMP; ++l) ptOrder[l] = l;
    for (int i = 0; i < nI; ++i) linkOrder[i] = i;
#ifdef FIB_ORACLE_REVERSE
    std::reverse(ptOrder.begin(), ptOrder.end()); std::reverse(linkOrder.begin(), linkOrder.end());
#endif
    byPoint.assign(nMP, {});
    for (int e = 0; e < nE; ++e) byPoint[eMP[e]].push_back(e);
    InfoI.assign((size_t)nI * 81, 0.0); InfoG.assign((size_t)nI * 9, 0.0); InfoA.assign((size_t)nI * 9, 0.0);
    for (int i = 0; i < nI; ++i) {
      inertial_information(pre[i].C, &InfoI[(size_t)i * 81]);
      double Cg[9], Ca[9];
      for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { Cg[r * 3 + c] = pre[i].C[(9 + r) * 15 + 9 + c]; Ca[r * 3 + c] = pre[i].C[(12 + r) * 15 + 12 + c]; }
      if (!invert(Cg, 3, &InfoG[(size_t)i * 9])) std::fill_n(&InfoG[(size_t)i * 9], 9, 0.0);
      if (!invert(Ca, 3, &InfoA[(size_t)i * 9])) std::fill_n(&InfoA[(size_t)i * 9], 9, 0.0);
    }
    vErr.assign((size_t)nE * 3, 0.0); iErr.assign((size_t)nI * 9, 0.0); gErr.assign((size_t)nI * 3, 0.0); aErr.assign((size_t)nI * 3, 0.0);
    // the envelope: a keyframe's rows begin at the first row of the lowest keyframe of the system it shares a point or a link with; the
    // shared biases' rows at the lowest keyframe that enters a link
    std::vector<int> firstOff(nKF, -1);
    for (int k : sys) firstOff[k] = S[k].off;
    for (int l = 0; l < nMP; ++l) {
      int lo = -1;
      for (int e : byPoint[l]) if (S[eKF[e]].off >= 0 && (lo < 0 || S[eKF[e]].off < lo)) lo = S[eKF[e]].off;
      for (int e : byPoint[l]) if (S[eKF[e]].off >= 0) firstOff[eKF[e]] = std::min(firstOff[eKF[e]], lo);
    }
    int sharedFirst = offB;
    for (int i = 0; i < nI; ++i) {
      const int a = S[iKF1[i]].off, c = S[iKF2[i]].off;
      if (a >= 0 && c >= 0) { const int hi = a > c ? iKF1[i] : iKF2[i]; firstOff[hi] = std::min(firstOff[hi], std::min(a, c)); }
      if (bInit && a >= 0) sharedFirst = std::min(sharedFirst, a);
      if (bInit && c >= 0) sharedFirst = std::min(sharedFirst, c);
    }
    firstScalar.assign(P, 0);
    for (int k : sys) for (int r = 0; r < S[k].wid; ++r) firstScalar[S[k].off + r] = firstOff[k];
    if (offB >= 0) for (int r = 0; r < 6; ++r) firstScalar[offB + r] = sharedFirst;
    nBlocks = 0;
    for (int r = 0; r < P; r += 3) nBlocks += (r - firstScalar[r]) / 3 + 1;
#ifdef FIB_ORACLE_DENSE
    std::fill(firstScalar.begin(), firstScalar.end(), 0);   // the whole lower triangle: a dense LDL^T without pivoting (nBlocks stays the envelope's)
#endif
    H.shape(firstScalar);
    b.assign((size_t)P + 3 * nMP, 0.0); Hll.assign((size_t)nMP * 9, 0.0); Hpl.assign((size_t)nE * 18, 0.0); x.assign((size_t)P + 3 * nMP, 0.0);
  }

  void computeErrors() {
    for (int e = 0; e < nE; ++e) vis_edge(g, S[eKF[e]], camOf(e), &pts[3 * eMP[e]], eObs + 3 * e, stereo(e), &vErr[3 * e], nullptr, nullptr);
    for (int i = 0; i < nI; ++i) {
      inertial_edge(pre[i], link_kf1(i), S[iKF2[i]], &iErr[9 * i], nullptr);
      for (int k = 0; k < 3; ++k) { gErr[3 * i + k] = S[iKF2[i]].bg[k] - S[iKF1[i]].bg[k]; aErr[3 * i + k] = S[iKF2[i]].ba[k] - S[iKF1[i]].ba[k]; }
    }
  }
  double robustChi2() const {
    double s = 0, w;
    for (int l : ptOrder) for (int e : byPoint[l]) s += huber(stereo(e) ? thStereo : thMono, visChi2(e), &w);
    for (int i : linkOrder) {
      s += huber(thInertial, quad(&iErr[9 * i], &InfoI[(size_t)i * 81], 9), &w);
      if (!bInit) s += quad(&gErr[3 * i], &InfoG[(size_t)i * 9], 3) + quad(&aErr[3 * i], &InfoA[(size_t)i * 9], 3);
    }
    if (bInit) {   // EdgePriorGyro, EdgePriorAcc: e = 0 - bias
      s += sb[0] * priorG * sb[0] + sb[1] * priorG * sb[1] + sb[2] * priorG * sb[2];
      s += sb[3] * priorA * sb[3] + sb[4] * priorA * sb[4] + sb[5] * priorA * sb[5];
    }
    return s;
  }
  void addH(int r, int c, double v) { if (r >= c) H.at(r, c) += v; }   // (the lower triangle; the upper one is its mirror)

  void buildSystem() {
    std::fill(H.v.begin(), H.v.end(), 0.0); std::fill(b.begin(), b.end(), 0.0); std::fill(Hll.begin(), Hll.end(), 0.0); std::fill(Hpl.begin(), Hpl.end(), 0.0);
    for (int l : ptOrder)
      for (int e : byPoint[l]) {
        const KF& K = S[eKF[e]];
        const bool st = stereo(e);
        const int d = st ? 3 : 2;
        const double info = eInv[e];
        double w, err[3], Jp[18], Jl[9];
        huber(st ? thStereo : thMono, visChi2(e), &w);
        vis_edge(g, K, camOf(e), &pts[3 * l], eObs + 3 * e, st, err, Jp, Jl);
        const double* er = &vErr[3 * e];
        for (int r = 0; r < 3; ++r) {
          double s = 0; for (int k = 0; k < d; ++k) s += Jl[k * 3 + r] * info * er[k];
          b[P + 3 * l + r] -= w * s;
          for (int c = 0; c < 3; ++c) { double h = 0; for (int k = 0; k < d; ++k) h += Jl[k * 3 + r] * (w * info) * Jl[k * 3 + c]; Hll[(size_t)l * 9 + r * 3 + c] += h; }
        }
        if (K.off < 0) continue;
        const int o = K.off;
        for (int r = 0; r < 6; ++r) {
          double s = 0; for (int k = 0; k < d; ++k) s += Jp[k * 6 + r] * info * er[k];
          b[o + r] -= w * s;
          for (int c = 0; c < 6; ++c) { double h = 0; for (int k = 0; k < d; ++k) h += Jp[k * 6 + r] * (w * info) * Jp[k * 6 + c]; addH(o + r, o + c, h); }
          for (int c = 0; c < 3; ++c) { double h = 0; for (int k = 0; k < d; ++k) h += Jp[k * 6 + r] * (w * info) * Jl[k * 3 + c]; Hpl[(size_t)e * 18 + r * 3 + c] = h; }
        }
      }
    for (int i : linkOrder) {
      const KF K1 = link_kf1(i);
      const KF &K1own = S[iKF1[i]], &K2 = S[iKF2[i]];
      double err[9], J[216], w = 1.0;
      inertial_edge(pre[i], K1, K2, err, J);
      const double* Om = &InfoI[(size_t)i * 81];
      const double* er = &iErr[9 * i];
      huber(thInertial, quad(er, Om, 9), &w);
      int colOf[24];   // edge column -> system column (-1: fixed vertex, or a vertex the keyframe's width leaves out)
      for (int a = 0; a < 15; ++a) colOf[a] = K1own.off >= 0 && a < K1own.wid ? K1own.off + a : -1;
      if (bInit) for (int a = 0; a < 6; ++a) colOf[9 + a] = offB + a;
      for (int a = 0; a < 9; ++a) colOf[15 + a] = K2.off >= 0 && a < K2.wid ? K2.off + a : -1;
      for (int a = 0; a < 24; ++a) {
        if (colOf[a] < 0) continue;
        double JtO[9], s = 0;
        for (int c = 0; c < 9; ++c) { double t = 0; for (int k = 0; k < 9; ++k) t += J[k * 24 + a] * Om[k * 9 + c]; JtO[c] = t; }
        for (int k = 0; k < 9; ++k) s += JtO[k] * er[k];
        b[colOf[a]] -= w * s;
        for (int c = 0; c < 24; ++c) {
          if (colOf[c] < 0) continue;
          double h = 0; for (int k = 0; k < 9; ++k) h += JtO[k] * J[k * 24 + c];
          addH(colOf[a], colOf[c], w * h);
        }
      }
      if (bInit) continue;
      for (int t = 0; t < 2; ++t) {   // EdgeGyroRW / EdgeAccRW: e = bias2 - bias1
        const double* Q = t == 0 ? &InfoG[(size_t)i * 9] : &InfoA[(size_t)i * 9];
        const double* e3 = t == 0 ? &gErr[3 * i] : &aErr[3 * i];
        const int o1 = K1own.wid == 15 ? K1own.off + 9 + 3 * t : -1, o2 = K2.wid == 15 ? K2.off + 9 + 3 * t : -1;
        for (int r = 0; r < 3; ++r) {
          double s = 0; for (int k = 0; k < 3; ++k) s += Q[r * 3 + k] * e3[k];
          if (o2 >= 0) b[o2 + r] -= s;
          if (o1 >= 0) b[o1 + r] += s;
          for (int c = 0; c < 3; ++c) {
            const double v = Q[r * 3 + c];
            if (o2 >= 0) addH(o2 + r, o2 + c, v);
            if (o1 >= 0) addH(o1 + r, o1 + c, v);
            if (o1 >= 0 && o2 >= 0) { addH(o1 + r, o2 + c, -v); addH(o2 + r, o1 + c, -v); }
          }
        }
      }
    }
    if (bInit && offB >= 0)   // the priors: information prior * I, d e / d bias = -I as e = 0 - bias demands
      for (int r = 0; r < 3; ++r) {
        addH(offB + r, offB + r, priorG); b[offB + r] -= priorG * sb[r];
        addH(offB + 3 + r, offB + 3 + r, priorA); b[offB + 3 + r] -= priorA * sb[3 + r];
      }
  }

  bool solveSystem(double lam) {   // the points behind the Schur complement, skyline LDL^T, back-substitution; a failed one leaves the step zero
    Skyline Hs = H;
    std::vector<double> bs(b.begin(), b.begin() + P), Dinv((size_t)nMP * 9);
    for (int i = 0; i < P; ++i) Hs.at(i, i) += lam;
    for (int l : ptOrder) {
      double D[9];
      memcpy(D, &Hll[(size_t)l * 9], sizeof D);
      D[0] += lam; D[4] += lam; D[8] += lam;
      double* Di = &Dinv[(size_t)l * 9];
      if (!invert(D, 3, Di)) memset(Di, 0, sizeof D);
      double db[3];
      for (int r = 0; r < 3; ++r) db[r] = Di[r * 3] * b[P + 3 * l] + Di[r * 3 + 1] * b[P + 3 * l + 1] + Di[r * 3 + 2] * b[P + 3 * l + 2];
      for (int e1 : byPoint[l]) {
        const int o1 = S[eKF[e1]].off;
        if (o1 < 0) continue;
        const double* B1 = &Hpl[(size_t)e1 * 18];
        double BD[18];
        for (int r = 0; r < 6; ++r) for (int c = 0; c < 3; ++c) BD[r * 3 + c] = B1[r * 3] * Di[c] + B1[r * 3 + 1] * Di[3 + c] + B1[r * 3 + 2] * Di[6 + c];
        for (int r = 0; r < 6; ++r) bs[o1 + r] -= B1[r * 3] * db[0] + B1[r * 3 + 1] * db[1] + B1[r * 3 + 2] * db[2];
        for (int e2 : byPoint[l]) {
          const int o2 = S[eKF[e2]].off;
          if (o2 < 0) continue;
          const double* B2 = &Hpl[(size_t)e2 * 18];
          for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c)
              if (o1 + r >= o2 + c) Hs.at(o1 + r, o2 + c) -= BD[r * 3] * B2[c * 3] + BD[r * 3 + 1] * B2[c * 3 + 1] + BD[r * 3 + 2] * B2[c * 3 + 2];
        }
      }
    }
    std::fill(x.begin(), x.end(), 0.0);
    if (!skyline_ldlt_solve(Hs, bs.data(), x.data())) { std::fill(x.begin(), x.end(), 0.0); return false; }
    for (int l = 0; l < nMP; ++l) {
      double cl[3] = {b[P + 3 * l], b[P + 3 * l + 1], b[P + 3 * l + 2]};
      for (int e : byPoint[l]) {
        const int o1 = S[eKF[e]].off;
        if (o1 < 0) continue;
        const double* B = &Hpl[(size_t)e * 18];
        for (int c = 0; c < 3; ++c) for (int r = 0; r < 6; ++r) cl[c] -= B[r * 3 + c] * x[o1 + r];
      }
      const double* Di = &Dinv[(size_t)l * 9];
      for (int r = 0; r < 3; ++r) x[P + 3 * l + r] = Di[r * 3] * cl[0] + Di[r * 3 + 1] * cl[1] + Di[r * 3 + 2] * cl[2];
    }
    return true;
  }
  void update(const double* dx) {
    for (KF& K : S) if (K.off >= 0) K.oplus(g, dx + K.off, K.wid);
    if (offB >= 0) for (int k = 0; k < 6; ++k) sb[k] += dx[offB + k];
    for (int k = 0; k < 3 * nMP; ++k) pts[k] += dx[P + k];
  }
};

}  // namespace

extern "C" {

// plan6 = {its, bInit, priorG, priorA, stop at entry, -}.  Outputs as the entries': kfState21 / mpPos / bias6 in place, stats4 = {outer
// iterations, trials, scalar unknowns of the reduced system, 3 x 3 envelope blocks}, chi2 = the robust chi2 before and after; info4 = {the
// solve ended on a rejected trial, ended by the stagnation rule, a factorisation failed, edges above their Huber bar at entry}.
void fib_oracle_run(int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos, int nE, const int* eKF, const int* eMP,
                    const float* eObs, const uint8_t* eRight, const float* eInvSigma2, int nI, const int* iKF1, const int* iKF2,
                    const float* iPre310, const float* cam5, const float* rig28, const float* Tbc12, const double* plan6, float* bias6,
                    int* stats4, double* chi2, int* info4) {
  memset(info4, 0, 16);
  stats4[0] = stats4[1] = stats4[2] = stats4[3] = 0;
  chi2[0] = chi2[1] = 0;
  const int its = (int)plan6[0];
  Problem Q;
  Q.setup(nKF, kfState21, kfKind, nMP, mpPos, nE, eKF, eMP, eObs, eRight, eInvSigma2, nI, iKF1, iKF2, iPre310, cam5, rig28, Tbc12, (int)plan6[1],
          plan6[2], plan6[3], bias6);
  if (!Q.P || plan6[4] != 0) return;
  const int P = Q.P;
  Q.computeErrors();
  {
    double w;
    for (int e = 0; e < nE; ++e) { huber(Q.stereo(e) ? Q.thStereo : Q.thMono, Q.visChi2(e), &w); if (w != 1.0) ++info4[3]; }
    for (int i = 0; i < nI; ++i) { huber(Q.thInertial, Problem::quad(&Q.iErr[9 * i], &Q.InfoI[(size_t)i * 81], 9), &w); if (w != 1.0) ++info4[3]; }
  }
  chi2[0] = chi2[1] = Q.robustChi2();
  double lambda = 1e-5, ni = 2;   // setUserLambdaInit(1e-5)
  int nBad = 0, trials = 0, outer = 0;
  bool lastRejected = false;
  for (int it = 0; it < its; ++it) {
    ++outer;
    Q.computeErrors();
    double currentChi = Q.robustChi2(), tempChi = currentChi;
    const double iniChi = currentChi;
    Q.buildSystem();
    double rho = 0;
    int qmax = 0;
    do {
      const std::vector<KF> Sbk = Q.S;
      const std::vector<double> ptsBk = Q.pts;
      double sbBk[6];
      memcpy(sbBk, Q.sb, sizeof sbBk);
      const bool ok = Q.solveSystem(lambda);
      if (!ok) info4[2] = 1;
      Q.update(Q.x.data());
      Q.computeErrors();
      tempChi = Q.robustChi2();
      if (!ok) tempChi = std::numeric_limits<double>::max();
      double scale = 0;
      for (size_t j = 0; j < Q.x.size(); ++j) scale += Q.x[j] * (lambda * Q.x[j] + Q.b[j]);
      rho = (currentChi - tempChi) / (scale + 1e-3);
      lastRejected = !(rho > 0 && std::isfinite(tempChi));
      if (!lastRejected) {
        double alpha = 1. - std::pow((2 * rho - 1), 3);
        alpha = std::min(alpha, 2. / 3.);
        lambda *= std::max(1. / 3., alpha);
        ni = 2;
        currentChi = tempChi;
      } else {
        lambda *= ni; ni *= 2;
        Q.S = Sbk; Q.pts = ptsBk; memcpy(Q.sb, sbBk, sizeof sbBk);
      }
      ++qmax; ++trials;
    } while (rho < 0 && qmax < 10);
    chi2[1] = currentChi;
    if (qmax == 10 || rho == 0 || rho != rho) break;
    if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
    if (nBad >= 3) { info4[1] = 1; break; }
  }
  info4[0] = lastRejected ? 1 : 0;
  stats4[0] = outer; stats4[1] = trials; stats4[2] = P; stats4[3] = Q.nBlocks;
  for (int k = 0; k < nKF; ++k) {
    if (Q.S[k].off < 0) continue;
    double s[21];
    Q.S[k].store(s);
    if (Q.S[k].wid == 9) for (int i = 0; i < 6; ++i) s[15 + i] = Q.sb[i];   // every bImu keyframe gets the shared biases (:719-738)
    for (int i = 0; i < (Q.S[k].wid == 6 ? 12 : 21); ++i) kfState21[21 * k + i] = (float)s[i];
  }
  if (Q.bInit) for (int k = 0; k < 6; ++k) bias6[k] = (float)Q.sb[k];
  for (int l = 0; l < nMP; ++l) if (!Q.byPoint[l].empty()) for (int k = 0; k < 3; ++k) mpPos[3 * l + k] = (float)Q.pts[3 * l + k];
}

// The first system's right-hand side b [P + 3 nMP] and the central-difference gradient of the robust chi2 along every unknown (through
// oplus, step h); returns P, or -(P + 1) when an edge starts above its Huber bar (the robustified b is then not the gradient's half).
int fib_oracle_gradient(int nKF, const float* kfState21, const uint8_t* kfKind, int nMP, const float* mpPos, int nE, const int* eKF, const int* eMP,
                        const float* eObs, const uint8_t* eRight, const float* eInvSigma2, int nI, const int* iKF1, const int* iKF2,
                        const float* iPre310, const float* cam5, const float* rig28, const float* Tbc12, const double* plan6, const float* bias6,
                        double h, double* bOut, double* gradOut) {
  Problem Q;
  Q.setup(nKF, kfState21, kfKind, nMP, mpPos, nE, eKF, eMP, eObs, eRight, eInvSigma2, nI, iKF1, iKF2, iPre310, cam5, rig28, Tbc12, (int)plan6[1],
          plan6[2], plan6[3], bias6);
  Q.computeErrors();
  int above = 0;
  double w;
  for (int e = 0; e < nE; ++e) { huber(Q.stereo(e) ? Q.thStereo : Q.thMono, Q.visChi2(e), &w); if (w != 1.0) ++above; }
  for (int i = 0; i < nI; ++i) { huber(Q.thInertial, Problem::quad(&Q.iErr[9 * i], &Q.InfoI[(size_t)i * 81], 9), &w); if (w != 1.0) ++above; }
  Q.buildSystem();
  const int N = Q.P + 3 * nMP;
  for (int j = 0; j < N; ++j) bOut[j] = Q.b[j];
  const std::vector<KF> S0 = Q.S;
  const std::vector<double> pts0 = Q.pts;
  double sb0[6];
  memcpy(sb0, Q.sb, sizeof sb0);
  std::vector<double> dx(N, 0.0);
  for (int j = 0; j < N; ++j) {
    double c[2];
    for (int s = 0; s < 2; ++s) {
      dx[j] = s ? -h : h;
      Q.update(dx.data());
      Q.computeErrors();
      c[s] = Q.robustChi2();
      Q.S = S0; Q.pts = pts0; memcpy(Q.sb, sb0, sizeof sb0);
    }
    dx[j] = 0;
    gradOut[j] = (c[0] - c[1]) / (2 * h);
  }
  return above ? -(Q.P + 1) : Q.P;
}

}  // extern "C"
