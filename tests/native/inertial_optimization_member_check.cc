// The three reference-typed Optimizer::InertialOptimization members of include/morb/Optimizer.h on mock keyframes
// (tests/native/mock_inertial_optimization), with the argument lists of the reference's three call sites in this project's own words:
//   LocalMapping::InitializeIMU:    InertialOptimization(map, mRwg, mScale, mbg, mba, mbMonocular, infoInertial, false, false, priorG, priorA)
//   LocalMapping::ScaleRefinement:  InertialOptimization(map, mRwg, mScale)
//   LoopClosing (map merge):        InertialOptimization(map, bg, ba)
// Run as `inertial_optimization_member_check <dir>`: reads kf_state / pre / global16 / prior2 / cfg (.bin) of one scene, builds the keyframes in
// SHUFFLED map order with one keyframe beyond GetMaxKFid(), calls the first overload and dumps what it wrote back in temporal order; then
// the other two overloads on the result.  The CPU suite compiles it to an object and looks for the three members there.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "inertial_optimization_mock.h"
#include "Optimizer.h"

using namespace ORB_SLAM3;

static std::string g_dir;
template <class T> static std::vector<T> load(const char* name) {
  std::ifstream f(g_dir + "/" + name + ".bin", std::ios::binary | std::ios::ate);
  if (!f) { std::printf("cannot open %s\n", name); std::exit(2); }
  const size_t n = (size_t)f.tellg();
  std::vector<T> v(n / sizeof(T));
  f.seekg(0); f.read(reinterpret_cast<char*>(v.data()), n);
  return v;
}
template <class T> static void dump(const char* name, const T* p, size_t n) {
  std::ofstream f(g_dir + "/out_" + name + ".bin", std::ios::binary);
  f.write(reinterpret_cast<const char*>(p), n * sizeof(T));
}

// the three members, instantiated whether or not main runs them (the CPU suite looks for them in the object file)
template void Optimizer::InertialOptimization<IOMap, Eigen::Matrix3d, Eigen::Vector3d, MatrixXd>(IOMap*, Eigen::Matrix3d&, double&, Eigen::Vector3d&,
                                                                                                 Eigen::Vector3d&, bool, MatrixXd&, bool, bool, float, float);
template void Optimizer::InertialOptimization<IOMap, Eigen::Vector3d>(IOMap*, Eigen::Vector3d&, Eigen::Vector3d&, float, float);
template void Optimizer::InertialOptimization<IOMap, Eigen::Matrix3d>(IOMap*, Eigen::Matrix3d&, double&);

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: %s <dir>\n", argv[0]); return 2; }
  g_dir = argv[1];
  const auto st = load<float>("kf_state"), pre = load<float>("pre"), prior2 = load<float>("prior2");
  const auto g16 = load<double>("global16");
  const auto cfg = load<int>("cfg");   // n, flags
  const int n = cfg[0];
  const size_t PF = sizeof(morb_imu_preintegrated) / sizeof(float);
  std::vector<IOKeyFrame> kfs(n + 1);
  std::vector<IOPreintegrated> pis(n + 1);
  for (int k = 0; k <= n; ++k) {
    IOKeyFrame& K = kfs[k];
    const float* s = &st[(size_t)21 * (k < n ? k : n - 1)];
    K.mnId = 10 + 2 * k;
    for (int q = 0; q < 9; ++q) K.mRwb.m[q] = s[q];
    for (int q = 0; q < 3; ++q) { K.mOwb(q) = s[9 + q]; K.mVw(q) = s[12 + q]; }
    K.mImuBias = IMU::Bias(s[18], s[19], s[20], s[15], s[16], s[17]);
    if (k == 0) continue;
    K.mPrevKF = &kfs[k - 1];
    K.mpImuPreintegrated = &pis[k];
    const float* p = &pre[PF * (k < n ? k : n - 1)];
    morb_imu_preintegrated r;
    std::memcpy(&r, p, sizeof r);
    IOPreintegrated& I = pis[k];
    I.dT = r.dT;
    for (int q = 0; q < 9; ++q) { I.dR.m[q] = r.dR[q]; I.JRg.m[q] = r.JRg[q]; I.JVg.m[q] = r.JVg[q]; I.JVa.m[q] = r.JVa[q]; I.JPg.m[q] = r.JPg[q]; I.JPa.m[q] = r.JPa[q]; }
    for (int q = 0; q < 3; ++q) { I.dV(q) = r.dV[q]; I.dP(q) = r.dP[q]; I.avgA(q) = r.avgA[q]; I.avgW(q) = r.avgW[q]; }
    for (int q = 0; q < 225; ++q) I.C.m[q] = r.C[q];
    I.b = IMU::Bias(r.b[0], r.b[1], r.b[2], r.b[3], r.b[4], r.b[5]);
    for (int q = 0; q < 6; ++q) { I.Nga.d(q) = r.nga[q]; I.NgaWalk.d(q) = r.ngaWalk[q]; }
  }
  IOMap map;
  map.maxKFid = kfs[n - 1].mnId;                    // the last keyframe (index n) is beyond it: dropped with its link
  map.keyframes.push_back(&kfs[0]);                 // vpKFs.front(): its bias is the initial bias
  {  // the others in a shuffled order
    std::vector<char> seen(n + 1, 0);
    seen[0] = 1;
    for (int k = 1; k <= n; ++k) { int j = (k * 7) % (n + 1); while (seen[j]) j = (j + 1) % (n + 1); seen[j] = 1; map.keyframes.push_back(&kfs[j]); }
  }

  Eigen::Matrix3d mRwg; Eigen::Vector3d mbg, mba;
  for (int q = 0; q < 9; ++q) mRwg.m[q] = g16[q];
  double mScale = g16[9];
  MatrixXd infoInertial;
  const bool mbMonocular = (cfg[1] & 1) != 0;
  const float priorG = prior2[0], priorA = prior2[1];
  Optimizer::InertialOptimization(&map, mRwg, mScale, mbg, mba, mbMonocular, infoInertial, false, false, priorG, priorA);

  std::vector<float> vb((size_t)9 * n);
  std::vector<int> re(n);
  for (int k = 0; k < n; ++k) {
    for (int q = 0; q < 3; ++q) vb[9 * k + q] = kfs[k].mVw(q);
    const IMU::Bias b = kfs[k].mImuBias;
    vb[9 * k + 3] = b.bwx; vb[9 * k + 4] = b.bwy; vb[9 * k + 5] = b.bwz; vb[9 * k + 6] = b.bax; vb[9 * k + 7] = b.bay; vb[9 * k + 8] = b.baz;
    re[k] = k ? pis[k].nReintegrated : 0;
    if (k && pis[k].nSetNewBias != 1) { std::printf("SetNewBias calls on link %d: %d\n", k, pis[k].nSetNewBias); return 1; }
  }
  if (pis[n].nReintegrated || pis[n].nSetNewBias || kfs[n].mVw(0) != st[(size_t)21 * (n - 1) + 12]) { std::printf("the keyframe beyond GetMaxKFid() was touched\n"); return 1; }
  double out16[16];
  for (int q = 0; q < 9; ++q) out16[q] = mRwg.m[q];
  out16[9] = mScale;
  for (int q = 0; q < 3; ++q) { out16[10 + q] = mbg(q); out16[13 + q] = mba(q); }
  dump("vel_bias", vb.data(), vb.size()); dump("reintegrated", re.data(), re.size()); dump("global16", out16, 16);

  {  // LoopClosing's call after a merge
    Eigen::Vector3d bg, ba;
    Optimizer::InertialOptimization(&map, bg, ba);
    double o[16] = {0};
    for (int q = 0; q < 3; ++q) { o[10 + q] = bg(q); o[13 + q] = ba(q); }
    dump("global16_mode1", o, 16);
  }
  {  // LocalMapping::ScaleRefinement
    Eigen::Matrix3d R; for (int q = 0; q < 9; ++q) R.m[q] = q % 4 == 0 ? 1.0 : 0.0;
    double s = 1.0;
    const float v0 = kfs[3].mVw(0);
    Optimizer::InertialOptimization(&map, R, s);
    if (kfs[3].mVw(0) != v0) { std::printf("the (Rwg, scale) overload wrote a velocity\n"); return 1; }
    double o[16] = {0};
    for (int q = 0; q < 9; ++q) o[q] = R.m[q];
    o[9] = s;
    dump("global16_mode2", o, 16);
  }
  std::printf("inertial optimization member ok\n");
  return 0;
}
