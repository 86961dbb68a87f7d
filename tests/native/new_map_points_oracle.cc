// CPU oracle of the body of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:489-709): one thread, a loop over the
// pairs and over each pair's matches in ascending idx1, as the reference visits vMatchedIndices.  Per match it calls
// include/morb/new_map_points_math.h, the header the kernel compiles too, so the arithmetic exists once; what is the oracle's own is
// the order, the counters, the tables and the AddMapPoint marks.  Built by tests/new_map_points_oracle.py with g++ -O2
// -ffp-contract=off (and a second time with -O3 -march=native -ffp-contract=fast, to show that no decision of the corpus sits on a
// rounding edge) and loaded with ctypes.
#include <cstdint>
#include <cstring>

#include "morb/new_map_points_math.h"
#include "morb_hip.h"

using namespace morbnmp;

namespace {

#define MORB_NMP_X(n) #n ","
const char kStatusNames[] = MORB_NMP_STATUS(MORB_NMP_X);
const char kStatNames[] = MORB_NMP_STATS(MORB_NMP_X);
#undef MORB_NMP_X

Camera camera(int kb8, const float* p8) {
  Camera c;
  c.kb8 = kb8;
  for (int i = 0; i < 8; ++i) c.p[i] = p8[i];
  return c;
}

}  // namespace

extern "C" {

const char* new_map_points_oracle_status_names() { return kStatusNames; }
const char* new_map_points_oracle_stat_names() { return kStatNames; }

int new_map_points_oracle_triangulate(const float* x_c1, const float* x_c2, const float* Tc1w, const float* Tc2w, float* x3D) {
  return nmp_triangulate(x_c1, x_c2, Tc1w, Tc2w, x3D) ? 1 : 0;
}

int new_map_points_oracle_gate(int monocular, const float* Ow1, const float* Ow2, float mb2, float medianDepthKF2) {
  return nmp_pair_gate(monocular != 0, Ow1, Ow2, mb2, medianDepthKF2) ? 1 : 0;
}

// One match from flat arrays.  cam: fx fy cx cy mb mbf; lm: ratioFactor thFarPoints; flags: inertial farPoints; per side s (0, 1):
// T[s] = Tcw (12) then Twc (12), Ow[s] (3), f[s] = x y rawx rawy ur depth, i[s] = octave bStereo kb8, cam8[s] (8).
int new_map_points_oracle_decide(const float* cam, const float* lm, const int* flags, const float* scaleFactors, const float* levelSigma2,
                                 const float* T, const float* Ow, const float* f, const int* i, const float* cam8, float* x3D,
                                 int* stereoFlags) {
  Params P;
  P.fx = cam[0]; P.fy = cam[1]; P.cx = cam[2]; P.cy = cam[3];
  P.invfx = 1.0f / P.fx; P.invfy = 1.0f / P.fy;
  P.mb = cam[4]; P.mbf = cam[5];
  P.ratioFactor = lm[0]; P.thFarPoints = lm[1];
  P.inertial = flags[0]; P.farPoints = flags[1];
  P.scaleFactors = scaleFactors; P.levelSigma2 = levelSigma2;
  Side s[2];
  for (int k = 0; k < 2; ++k) {
    s[k].Tcw = T + 24 * k; s[k].Twc = T + 24 * k + 12;
    for (int c = 0; c < 3; ++c) s[k].Ow[c] = Ow[3 * k + c];
    s[k].x = f[6 * k]; s[k].y = f[6 * k + 1]; s[k].rawx = f[6 * k + 2]; s[k].rawy = f[6 * k + 3]; s[k].ur = f[6 * k + 4];
    s[k].depth = f[6 * k + 5];
    s[k].octave = i[3 * k]; s[k].bStereo = i[3 * k + 1];
    s[k].cam = camera(i[3 * k + 2], cam8 + 8 * k);
  }
  return nmp_decide(P, s[0], s[1], x3D, stereoFlags);
}

// The batched entry points' arguments, host arrays throughout; cam6 = fx fy cx cy mb mbf.  nLeft1 == NULL: pinhole keyframes.
void new_map_points_oracle_run(int npairs, const int* img1, const int* img2, const int* nLeft1, const int* nLeft2, int nimg, int cap,
                               const int* count, const morb_keypoint* kps, const morb_keypoint* kpsRaw, const uint8_t* desc,
                               const float* uRight, const float* depth, const float* cam6, int nlevels, const float* scaleFactors,
                               const float* levelSigma2, const float* camL8, const float* camR8, const int* match12, const float* poses,
                               const uint8_t* kf2First, float ratioFactor, int mbInertial, int mbFarPoints, float mThFarPoints, int* status,
                               int* stats, int nrows, const int* row, float* Xw, float* normal, float* maxDist, float* minDist,
                               uint8_t* mpDesc, int* obsImg2, int* obsIdx2, uint8_t* hasMP) {
  const bool rig = nLeft1 != nullptr;
  Params P;
  P.fx = cam6[0]; P.fy = cam6[1]; P.cx = cam6[2]; P.cy = cam6[3];
  P.invfx = 1.0f / P.fx; P.invfy = 1.0f / P.fy;
  P.mb = cam6[4]; P.mbf = cam6[5];
  P.ratioFactor = ratioFactor; P.thFarPoints = mThFarPoints;
  P.inertial = mbInertial ? 1 : 0; P.farPoints = mbFarPoints ? 1 : 0;
  P.scaleFactors = scaleFactors; P.levelSigma2 = levelSigma2;
  const float K8[8] = {P.fx, P.fy, P.cx, P.cy, 0, 0, 0, 0};
  const Camera cL = camera(rig, rig ? camL8 : K8), cR = camera(rig, rig ? camR8 : K8);
  const int nposes = rig ? NMP_PAIR_POSES_RIG : NMP_PAIR_POSES;
  for (int p = 0; p < npairs; ++p) {
    int* st = status + (size_t)p * cap;
    int* S = stats + (size_t)p * NMP_STATS_LEN;
    for (int i = 0; i < cap; ++i) st[i] = NMP_NONE;
    const int a = img1[p], b = img2[p], r = row[p];
    if (a < 0 || a >= nimg || b < 0 || b >= nimg || r < 0 || r >= nrows) {
      for (int k = 0; k < NMP_STATS_LEN; ++k) S[k] = -1;
      continue;
    }
    for (int k = 0; k < NMP_STATS_LEN; ++k) S[k] = 0;
    const int n1 = count[a] < cap ? (count[a] > 0 ? count[a] : 0) : cap, n2 = count[b] < cap ? (count[b] > 0 ? count[b] : 0) : cap;
    const float* T = poses + (size_t)p * nposes * NMP_POSE;
    const size_t f1 = (size_t)a * cap, f2 = (size_t)b * cap;
    for (int i1 = 0; i1 < n1; ++i1) {
      const int i2 = match12[(size_t)p * cap + i1];
      if (i2 < 0 || i2 >= n2) continue;
      const bool right1 = rig && i1 >= nLeft1[p], right2 = rig && i2 >= nLeft2[p];
      const float* T1 = T + (right1 ? 2 : 0) * NMP_POSE;
      const float* T2 = T + ((rig ? 4 : 2) + (right2 ? 2 : 0)) * NMP_POSE;
      Side s1, s2;
      s1.Tcw = T1; s1.Twc = T1 + NMP_POSE;
      s2.Tcw = T2; s2.Twc = T2 + NMP_POSE;
      for (int c = 0; c < 3; ++c) { s1.Ow[c] = s1.Twc[4 * c + 3]; s2.Ow[c] = s2.Twc[4 * c + 3]; }
      s1.cam = right1 ? cR : cL;
      s2.cam = right2 ? cR : cL;
      const morb_keypoint &kp1 = kps[f1 + i1], &kp2 = kps[f2 + i2];
      auto level = [&](int o) { return o < 0 ? 0 : (o >= nlevels ? nlevels - 1 : o); };
      s1.x = kp1.x; s1.y = kp1.y; s1.octave = level(kp1.octave);
      s2.x = kp2.x; s2.y = kp2.y; s2.octave = level(kp2.octave);
      const morb_keypoint* raw = kpsRaw ? kpsRaw : kps;
      s1.rawx = raw[f1 + i1].x; s1.rawy = raw[f1 + i1].y;
      s2.rawx = raw[f2 + i2].x; s2.rawy = raw[f2 + i2].y;
      const bool stereo = !rig && uRight;
      s1.ur = stereo ? uRight[f1 + i1] : -1.f; s1.depth = stereo ? depth[f1 + i1] : -1.f;
      s2.ur = stereo ? uRight[f2 + i2] : -1.f; s2.depth = stereo ? depth[f2 + i2] : -1.f;
      s1.bStereo = s1.ur >= 0; s2.bStereo = s2.ur >= 0;
      float x3D[3];
      int flags = 0;
      const int code = nmp_decide(P, s1, s2, x3D, &flags);
      st[i1] = code;
      if (flags & 1) S[NMP_S_TOTAL_STEREO_PTS]++;
      if (flags & 2) S[NMP_S_STEREO_ATTEMPT]++;
      if (flags & 4) S[NMP_S_STEREO_GOOD_PROJ]++;
      if (!nmp_created(code)) continue;
      S[NMP_S_CREATED]++;
      if (code != NMP_TRIANGULATED) S[NMP_S_COUNT_STEREO]++;
      const size_t o = (size_t)r * cap + i1;
      const float OwRef[3] = {T[NMP_POSE + 3], T[NMP_POSE + 7], T[NMP_POSE + 11]};
      nmp_point_fields(x3D, s1.Ow, s2.Ow, OwRef, scaleFactors[s1.octave], scaleFactors[nlevels - 1], normal + 3 * o, maxDist + o, minDist + o);
      for (int c = 0; c < 3; ++c) Xw[3 * o + c] = x3D[c];
      std::memcpy(mpDesc + 32 * o, desc + 32 * (nmp_descriptor_from_kf2(kf2First[p]) ? f2 + i2 : f1 + i1), 32);
      obsImg2[o] = b;
      obsIdx2[o] = i2;
      hasMP[f1 + i1] = 1;
      hasMP[f2 + i2] = 1;
    }
  }
}

}  // extern "C"
