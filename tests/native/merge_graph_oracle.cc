// CPU oracle of the second overload of Optimizer::OptimizeEssentialGraph (Optimizer.cc:1737-2063, map merging) on the flattened input of
// morb_optimize_essential_graph_merge (include/morb_hip.h): the preparation of :1783-1999 with the reference's quirks, the solver of
// essential_graph_oracle.cc (included: the same g2o restatement, the same builds), and the tail of :2015-2062 in float as Sophus computes it.
// The preparation follows the reference's own structure — the arrays vScw, vCorrectedSwc, vpGoodPose and vpBadPose filled list by list, then
// the edge loop over them — where the library recomputes each measurement from the poses of its two ends.
#include "essential_graph_oracle.cc"

namespace {

enum { IN_FIXED = 1, IN_CORRECTED = 2, IN_NONFIXED = 4 };

// Eigen's squaredNorm of four coefficients: the packets add (x^2, y^2) + (z^2, w^2), then the two lanes
template <class T> T norm4(const T* q) { return std::sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3])); }
template <class T> void so3_normalize(T* q) { const T n = norm4(q); for (int k = 0; k < 4; ++k) q[k] /= n; }

// Sophus::SE3d T = pose.cast<double>(); g2o::Sim3(T.unit_quaternion(), T.translation(), 1.0)
Sim3 sim3_of_pose(const float* p) {
  Sim3 S;
  for (int k = 0; k < 4; ++k) S.q[k] = (double)p[k];
  so3_normalize(S.q);
  for (int k = 0; k < 3; ++k) S.t[k] = (double)p[4 + k];
  S.s = 1.0;
  return S;
}

struct SE3f { float q[4], t[3]; };
SE3f se3f_load(const float* p) { SE3f T; memcpy(&T, p, sizeof T); return T; }
void so3f_rotate(const float* q, const float* p, float* o) {   // SO3::operator*(point)
  float uv[3] = {q[1] * p[2] - q[2] * p[1], q[2] * p[0] - q[0] * p[2], q[0] * p[1] - q[1] * p[0]};
  for (int k = 0; k < 3; ++k) uv[k] += uv[k];
  const float c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
  for (int k = 0; k < 3; ++k) o[k] = (p[k] + q[3] * uv[k]) + c[k];
}
SE3f se3f_inverse(const SE3f& T) {   // SO3 invR = so3().inverse(); SE3(invR, invR * (translation() * Scalar(-1)))
  SE3f r;
  for (int k = 0; k < 3; ++k) r.q[k] = -T.q[k];
  r.q[3] = T.q[3];
  so3_normalize(r.q);
  const float m[3] = {T.t[0] * -1.f, T.t[1] * -1.f, T.t[2] * -1.f};
  so3f_rotate(r.q, m, r.t);
  return r;
}
SE3f se3f_mul(const SE3f& A, const SE3f& B) {   // SE3(so3() * other.so3(), translation() + so3() * other.translation())
  SE3f r;
  const float *a = A.q, *b = B.q;
  r.q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  r.q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  r.q[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  r.q[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  so3_normalize(r.q);
  float rt[3];
  so3f_rotate(A.q, B.t, rt);
  for (int k = 0; k < 3; ++k) r.t[k] = A.t[k] + rt[k];
  return r;
}
SE3f se3f_of_sim3(const Sim3& S) {   // Sophus::SE3d Tiw(rotation(), translation() / s); Tiw.cast<float>()
  double q[4] = {S.q[0], S.q[1], S.q[2], S.q[3]};
  so3_normalize(q);
  SE3f T;
  for (int k = 0; k < 4; ++k) T.q[k] = (float)q[k];
  so3_normalize(T.q);
  for (int k = 0; k < 3; ++k) T.t[k] = (float)(S.t[k] / S.s);
  return T;
}

struct Prepared {
  std::vector<Sim3> est;             // the vertices' estimates
  std::vector<uint8_t> flags;        // bit 0 fixed, bit 1 _fix_scale
  std::vector<char> good, bad;       // vpGoodPose, vpBadPose
  std::vector<int> eI, eJ;
  std::vector<double> eS;
};

// :1783-1999 on the flattened lists
void prepare(int nKF, const uint8_t* lists, const float* Tcw, const float* TcwBef, int nC, const int* cI, const int* cJ, uint8_t* kept, Prepared& g) {
  std::vector<Sim3> vScw(nKF), vCorrectedSwc(nKF);
  const Sim3 identity = {{0, 0, 0, 1}, {0, 0, 0}, 1};
  for (int v = 0; v < nKF; ++v) vScw[v] = vCorrectedSwc[v] = identity;   // vector<g2o::Sim3>(nMaxKFid + 1)
  g.est.assign(nKF, identity); g.flags.assign(nKF, 0); g.good.assign(nKF, 0); g.bad.assign(nKF, 0);
  for (int v = 0; v < nKF; ++v) if (lists[v] & IN_FIXED) {   // vpFixedKFs
    const Sim3 Siw = sim3_of_pose(Tcw + v * 7);
    vCorrectedSwc[v] = inverse(Siw);
    g.est[v] = Siw; g.flags[v] = 3;
    g.good[v] = 1; g.bad[v] = 0;
  }
  std::vector<char> sIdKF(nKF, 0);
  for (int v = 0; v < nKF; ++v) if (lists[v] & IN_CORRECTED) {   // vpFixedCorrectedKFs
    const Sim3 Siw = sim3_of_pose(Tcw + v * 7);
    vCorrectedSwc[v] = inverse(Siw);
    g.est[v] = Siw; g.flags[v] = 1;
    vScw[v] = sim3_of_pose(TcwBef + v * 7);
    sIdKF[v] = 1;
    g.good[v] = 1; g.bad[v] = 1;
  }
  for (int v = 0; v < nKF; ++v) if (lists[v] & IN_NONFIXED) {   // vpNonFixedKFs
    if (sIdKF[v]) continue;
    const Sim3 Siw = sim3_of_pose(Tcw + v * 7);
    vScw[v] = Siw;
    g.est[v] = Siw; g.flags[v] = 0;
    g.good[v] = 0; g.bad[v] = 1;
  }
  for (int c = 0; c < nC; ++c) {
    const int i = cI[c], j = cJ[c];
    Sim3 Swi = identity;   // g2o::Sim3 Swi; (correctedSwi is never used)
    if (g.bad[i]) Swi = inverse(vScw[i]);
    Sim3 Sjw = identity;
    bool bHasRelation = false;
    if (g.good[i] && g.good[j]) { Sjw = inverse(vCorrectedSwc[j]); bHasRelation = true; }
    else if (g.bad[i] && g.bad[j]) { Sjw = vScw[j]; bHasRelation = true; }
    kept[c] = bHasRelation ? 1 : 0;
    if (!bHasRelation) continue;
    const Sim3 Sji = mul(Sjw, Swi);
    g.eI.push_back(i); g.eJ.push_back(j);
    g.eS.resize(g.eS.size() + 8);
    store(&g.eS[g.eS.size() - 8], Sji);
  }
}

}  // namespace

extern "C" {

// the preparation alone: kept[nC], est[nKF][8], flags[nKF], and the kept edges' eI, eJ, eS (room for nC each); returns their number
int mg_oracle_prepare(int nKF, const uint8_t* lists, const float* Tcw, const float* TcwBef, int nC, const int* cI, const int* cJ, uint8_t* kept,
                      double* est, uint8_t* flags, int* eI, int* eJ, double* eS) {
  Prepared g;
  prepare(nKF, lists, Tcw, TcwBef, nC, cI, cJ, kept, g);
  for (int v = 0; v < nKF; ++v) { store(est + (size_t)v * 8, g.est[v]); flags[v] = g.flags[v]; }
  for (size_t e = 0; e < g.eI.size(); ++e) { eI[e] = g.eI[e]; eJ[e] = g.eJ[e]; }
  if (!g.eS.empty()) memcpy(eS, g.eS.data(), sizeof(double) * g.eS.size());
  return (int)g.eI.size();
}

// the whole call, as morb_optimize_essential_graph_merge: the four pose arrays and the points in place
void mg_oracle_run(int nKF, const uint8_t* lists, float* Tcw, float* Twc, float* TcwBef, float* TwcBef, int nC, const int* cI, const int* cJ,
                   uint8_t* kept, int nMP, float* mp, const int* mpRef, int* stats4, double* chi2) {
  Prepared g;
  prepare(nKF, lists, Tcw, TcwBef, nC, cI, cJ, kept, g);
  std::vector<double> S((size_t)nKF * 8);
  for (int v = 0; v < nKF; ++v) store(&S[(size_t)v * 8], g.est[v]);
  eg_oracle_run(nKF, S.data(), g.flags.data(), (int)g.eI.size(), g.eI.data(), g.eJ.data(), g.eS.data(), 0, nullptr, nullptr, stats4, chi2);
  for (int v = 0; v < nKF; ++v) {   // :2015-2030
    if (!(lists[v] & IN_NONFIXED)) continue;
    const SE3f Tiw = se3f_of_sim3(load(&S[(size_t)v * 8]));
    memcpy(TcwBef + v * 7, Tcw + v * 7, sizeof(float) * 7);   // mTcwBefMerge = GetPose()
    memcpy(TwcBef + v * 7, Twc + v * 7, sizeof(float) * 7);   // mTwcBefMerge = GetPoseInverse()
    const SE3f Twi = se3f_inverse(Tiw);                       // SetPose: mTwc = mTcw.inverse()
    memcpy(Tcw + v * 7, &Tiw, sizeof(float) * 7);
    memcpy(Twc + v * 7, &Twi, sizeof(float) * 7);
  }
  for (int m = 0; m < nMP; ++m) {   // :2034-2062
    const int v = mpRef[m];
    if (v < 0 || !g.bad[v]) continue;
    const SE3f TNonCorrectedwr = se3f_load(TwcBef + v * 7), Twr = se3f_load(Twc + v * 7);
    const SE3f T = se3f_mul(Twr, se3f_inverse(TNonCorrectedwr));
    float r[3];
    so3f_rotate(T.q, mp + m * 3, r);
    for (int k = 0; k < 3; ++k) mp[m * 3 + k] = r[k] + T.t[k];
  }
}

}
