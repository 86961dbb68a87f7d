// The per-match arithmetic of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:569-690), GeometricTools::Triangulate
// (src/GeometricTools.cc:48-72), KeyFrame::UnprojectStereo (src/KeyFrame.cc:780-794) and the fields MapPoint::UpdateNormalAndDepth /
// ComputeDistinctiveDescriptors give a point of exactly two observations (src/MapPoint.cc:367-519), shared by the kernel
// (csrc/new_map_points.hip), the C++ adapter (include/morb/LocalMapping.h), the CPU oracle and the native checks: plain C++ that
// compiles for the host and for the device, written once so that the kernel and the oracle cannot drift apart.
//   * NewMapPointStatus: one code per `continue` of the reference's loop body and one per way a point is made;
//   * NewMapPointStat: the row morb_create_new_map_points_batch writes to d_stats;
//   * nmp_decide: the decision sequence of one match, float and double mixed exactly as the reference's expressions resolve;
//   * nmp_point_fields, nmp_descriptor_from_kf2: mNormalVector, mfMaxDistance, mfMinDistance and which descriptor wins;
//   * nmp_pair_gate (host): the baseline test in front of the search (:454-466).
// Conventions: a pose is a 3 x 4 row-major [R | t]; 3 x 3 products sum k = 0, 1, 2 left to right; the null vector
// of the 4 x 4 system, the two camera models and the float libm they call are camera_math.h's.
#pragma once
#include <cmath>
#include <cstdint>

#include "camera_math.h"

#if defined(__HIPCC__)
#define MORB_NMP_FN __host__ __device__ __forceinline__
#define MORB_NMP_UNROLL _Pragma("unroll")
#else
#define MORB_NMP_FN inline
#define MORB_NMP_UNROLL
#endif

// X(name): one list for the enum and for the Python front's tuple (matcher.NEW_MAP_POINT_STATUS)
#define MORB_NMP_STATUS(X)                                                                                      \
  X(NONE)               /* no match at this feature (match12 negative, or at or beyond keyframe 2's count) */     \
  X(TRIANGULATED)       /* created by Triangulate (:599) */                                                      \
  X(STEREO1)            /* created by mpCurrentKeyFrame->UnprojectStereo (:604) */                               \
  X(STEREO2)            /* created by pKF2->UnprojectStereo (:608) */                                            \
  X(LOW_PARALLAX)       /* no stereo and very low parallax (:610) */                                             \
  X(TRIANGULATE_FALSE)  /* Triangulate returned false: x3Dh(3) == 0 (:600) */                                    \
  X(UNPROJECT_FALSE)    /* UnprojectStereo returned false: depth <= 0 (:615) */                                  \
  X(Z1)                 /* z1 <= 0 (:619) */                                                                     \
  X(Z2)                 /* z2 <= 0 (:622) */                                                                     \
  X(REPROJ1)            /* reprojection error in the current keyframe (:635, :644) */                            \
  X(REPROJ2)            /* reprojection error in the neighbour (:658, :666) */                                   \
  X(ZERO_DIST)          /* dist1 == 0 || dist2 == 0 (:678) */                                                    \
  X(FAR_POINT)          /* mbFarPoints and a distance >= mThFarPoints (:680) */                                  \
  X(SCALE)              /* the scale-consistency test (:688) */

#define MORB_NMP_STATS(X) X(CREATED) X(TOTAL_STEREO_PTS) X(STEREO_ATTEMPT) X(STEREO_GOOD_PROJ) X(COUNT_STEREO)

namespace morbnmp {

#define MORB_NMP_X(n) NMP_##n,
enum NewMapPointStatus { MORB_NMP_STATUS(MORB_NMP_X) NMP_STATUS_LEN };
#undef MORB_NMP_X
#define MORB_NMP_X(n) NMP_S_##n,
enum NewMapPointStat { MORB_NMP_STATS(MORB_NMP_X) NMP_STATS_LEN };
#undef MORB_NMP_X

using morbcam::Camera;   // the camera of a Side, as this namespace's users name it

MORB_NMP_FN bool nmp_created(int status) { return status == NMP_TRIANGULATED || status == NMP_STEREO1 || status == NMP_STEREO2; }

constexpr int NMP_POSE = 12;              // floats of one 3 x 4 pose
constexpr int NMP_PAIR_POSES = 4;         // pinhole pair: Tcw1, Twc1, Tcw2, Twc2
constexpr int NMP_PAIR_POSES_RIG = 8;     // rig pair: Tcw1, Twc1, Trw1, Twr1, Tcw2, Twc2, Trw2, Twr2 (left pose, its inverse, right pose, its inverse)

// GeometricTools::Triangulate: x3Dh is a Vector4f, the test and the division are float
MORB_NMP_FN bool nmp_triangulate(const float* x_c1, const float* x_c2, const float* Tc1w, const float* Tc2w, float* x3D) {
  float A[16];
  MORB_NMP_UNROLL
  for (int k = 0; k < 4; ++k) {
    A[k] = x_c1[0] * Tc1w[8 + k] - Tc1w[k];
    A[4 + k] = x_c1[1] * Tc1w[8 + k] - Tc1w[4 + k];
    A[8 + k] = x_c2[0] * Tc2w[8 + k] - Tc2w[k];
    A[12 + k] = x_c2[1] * Tc2w[8 + k] - Tc2w[4 + k];
  }
  double xh[4];
  morbcam::null_vector4(A, xh);
  const float w = (float)xh[3];
  if (w == 0) return false;
  x3D[0] = (float)xh[0] / w; x3D[1] = (float)xh[1] / w; x3D[2] = (float)xh[2] / w;
  return true;
}

// KeyFrame::UnprojectStereo: (u, v) = mvKeys[i].pt (not mvKeysUn), Twc = the keyframe's own mTwc (mRwc is its rotation block)
MORB_NMP_FN bool nmp_unproject_stereo(float z, float u, float v, float cx, float cy, float invfx, float invfy, const float* Twc, float* x3D) {
  if (z > 0) {
    const float x = (u - cx) * z * invfx;
    const float y = (v - cy) * z * invfy;
    MORB_NMP_UNROLL
    for (int i = 0; i < 3; ++i) x3D[i] = ((Twc[i * 4] * x + Twc[i * 4 + 1] * y) + Twc[i * 4 + 2] * z) + Twc[i * 4 + 3];
    return true;
  }
  return false;
}

// What one match reads of one of its two keyframes.  Tcw / Ow: pose and centre of the camera that observes the feature (on a rig the
// right camera's for a right feature, :520-567).  Twc: the keyframe's own mTwc, read by UnprojectStereo only.
struct Side {
  const float* Tcw;
  const float* Twc;
  float Ow[3];
  Camera cam;
  float x, y;         // kp.pt: mvKeysUn[idx], or mvKeys / mvKeysRight on a rig
  int octave;
  float rawx, rawy;   // mvKeys[idx].pt
  float ur;           // mvuRight[idx]
  float depth;        // mvDepth[idx]
  int bStereo;        // !mpCamera2 && mvuRight[idx] >= 0
};

// Members of the two keyframes and of LocalMapping.  Every keyframe of a batch shares one camera (morb_frame_params), so fx1 == fx2 and so
// on; the comments in nmp_decide name the member the reference reads at each place.
struct Params {
  float fx, fy, cx, cy, invfx, invfy;   // invfx = 1.0f / fx (KeyFrame.cc:66)
  float mb, mbf;
  float ratioFactor;                    // 1.5f * mpCurrentKeyFrame->mfScaleFactor
  float thFarPoints;
  int inertial, farPoints;
  const float* scaleFactors;            // mvScaleFactors
  const float* levelSigma2;             // mvLevelSigma2
};

MORB_NMP_FN float nmp_row_dot(const float* T, int r, const float* x) { return ((T[r * 4] * x[0] + T[r * 4 + 1] * x[1]) + T[r * 4 + 2] * x[2]); }
MORB_NMP_FN float nmp_norm3(const float* v) { return sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

// LocalMapping.cc:569-690 for one match.  stereoFlags: bit 0 = counted in totalStereoPts, bit 1 = countStereoAttempt, bit 2 =
// countStereoGoodProj (countStereo = a created point whose status is NMP_STEREO1 / NMP_STEREO2).  x3D is the new point when the status
// is one of the three created codes.
MORB_NMP_FN int nmp_decide(const Params& P, const Side& s1, const Side& s2, float* x3D, int* stereoFlags) {
  const float* Tcw1 = s1.Tcw;
  const float* Tcw2 = s2.Tcw;
  float xn1[3], xn2[3], ray1[3], ray2[3];
  morbcam::unproject(s1.cam, s1.x, s1.y, xn1);
  morbcam::unproject(s2.cam, s2.x, s2.y, xn2);
  // ray = Rwc * xn with Rwc = Rcw.transpose()
  MORB_NMP_UNROLL
  for (int i = 0; i < 3; ++i) {
    ray1[i] = (Tcw1[i] * xn1[0] + Tcw1[4 + i] * xn1[1]) + Tcw1[8 + i] * xn1[2];
    ray2[i] = (Tcw2[i] * xn2[0] + Tcw2[4 + i] * xn2[1]) + Tcw2[8 + i] * xn2[2];
  }
  const float cosParallaxRays = ((ray1[0] * ray2[0] + ray1[1] * ray2[1]) + ray1[2] * ray2[2]) / (nmp_norm3(ray1) * nmp_norm3(ray2));

  float cosParallaxStereo = cosParallaxRays + 1;
  float cosParallaxStereo1 = cosParallaxStereo;
  float cosParallaxStereo2 = cosParallaxStereo;
  const bool bStereo1 = s1.bStereo != 0, bStereo2 = s2.bStereo != 0;
  // cos(2 * atan2(mb / 2, mvDepth[idx])): float overloads (mpCurrentKeyFrame->mb, then pKF2->mb)
  if (bStereo1)
    cosParallaxStereo1 = MORB_CAM_COSF(2 * MORB_CAM_ATAN2F(P.mb / 2, s1.depth));
  else if (bStereo2)
    cosParallaxStereo2 = MORB_CAM_COSF(2 * MORB_CAM_ATAN2F(P.mb / 2, s2.depth));
  int flags = (bStereo1 || bStereo2) ? 1 : 0;
  cosParallaxStereo = fminf(cosParallaxStereo1, cosParallaxStereo2);

  bool goodProj = false;
  bool bPointStereo = false;
  int made = NMP_TRIANGULATED;
  if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 &&
      (bStereo1 || bStereo2 || ((double)cosParallaxRays < 0.9996 && P.inertial) || ((double)cosParallaxRays < 0.9998 && !P.inertial))) {
    goodProj = nmp_triangulate(xn1, xn2, Tcw1, Tcw2, x3D);
    if (!goodProj) { *stereoFlags = flags; return NMP_TRIANGULATE_FALSE; }
  } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
    flags |= 2;
    bPointStereo = true;
    made = NMP_STEREO1;
    goodProj = nmp_unproject_stereo(s1.depth, s1.rawx, s1.rawy, P.cx, P.cy, P.invfx, P.invfy, s1.Twc, x3D);
  } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
    flags |= 2;
    bPointStereo = true;
    made = NMP_STEREO2;
    goodProj = nmp_unproject_stereo(s2.depth, s2.rawx, s2.rawy, P.cx, P.cy, P.invfx, P.invfy, s2.Twc, x3D);
  } else {
    *stereoFlags = flags;
    return NMP_LOW_PARALLAX;
  }
  if (goodProj && bPointStereo) flags |= 4;
  *stereoFlags = flags;
  if (!goodProj) return NMP_UNPROJECT_FALSE;

  // in front of both cameras
  const float z1 = nmp_row_dot(Tcw1, 2, x3D) + Tcw1[11];
  if (z1 <= 0) return NMP_Z1;
  const float z2 = nmp_row_dot(Tcw2, 2, x3D) + Tcw2[11];
  if (z2 <= 0) return NMP_Z2;

  // reprojection error in the first keyframe
  const float sigmaSquare1 = P.levelSigma2[s1.octave];
  const float x1 = nmp_row_dot(Tcw1, 0, x3D) + Tcw1[3];
  const float y1 = nmp_row_dot(Tcw1, 1, x3D) + Tcw1[7];
  const float invz1 = (float)(1.0 / (double)z1);
  if (!bStereo1) {
    const float Xc1[3] = {x1, y1, z1};
    float uv1[2];
    morbcam::project(s1.cam, Xc1, uv1[0], uv1[1]);
    const float errX1 = uv1[0] - s1.x;
    const float errY1 = uv1[1] - s1.y;
    if ((double)(errX1 * errX1 + errY1 * errY1) > 5.991 * (double)sigmaSquare1) return NMP_REPROJ1;
  } else {
    const float u1 = P.fx * x1 * invz1 + P.cx;
    const float u1_r = u1 - P.mbf * invz1;   // mpCurrentKeyFrame->mbf
    const float v1 = P.fy * y1 * invz1 + P.cy;
    const float errX1 = u1 - s1.x;
    const float errY1 = v1 - s1.y;
    const float errX1_r = u1_r - s1.ur;
    if ((double)((errX1 * errX1 + errY1 * errY1) + errX1_r * errX1_r) > 7.8 * (double)sigmaSquare1) return NMP_REPROJ1;
  }

  // ... in the second
  const float sigmaSquare2 = P.levelSigma2[s2.octave];
  const float x2 = nmp_row_dot(Tcw2, 0, x3D) + Tcw2[3];
  const float y2 = nmp_row_dot(Tcw2, 1, x3D) + Tcw2[7];
  const float invz2 = (float)(1.0 / (double)z2);
  if (!bStereo2) {
    const float Xc2[3] = {x2, y2, z2};
    float uv2[2];
    morbcam::project(s2.cam, Xc2, uv2[0], uv2[1]);
    const float errX2 = uv2[0] - s2.x;
    const float errY2 = uv2[1] - s2.y;
    if ((double)(errX2 * errX2 + errY2 * errY2) > 5.991 * (double)sigmaSquare2) return NMP_REPROJ2;
  } else {
    const float u2 = P.fx * x2 * invz2 + P.cx;
    const float u2_r = u2 - P.mbf * invz2;   // mpCurrentKeyFrame->mbf here too (:661)
    const float v2 = P.fy * y2 * invz2 + P.cy;
    const float errX2 = u2 - s2.x;
    const float errY2 = v2 - s2.y;
    const float errX2_r = u2_r - s2.ur;
    if ((double)((errX2 * errX2 + errY2 * errY2) + errX2_r * errX2_r) > 7.8 * (double)sigmaSquare2) return NMP_REPROJ2;
  }

  // scale consistency
  const float normal1[3] = {x3D[0] - s1.Ow[0], x3D[1] - s1.Ow[1], x3D[2] - s1.Ow[2]};
  const float dist1 = nmp_norm3(normal1);
  const float normal2[3] = {x3D[0] - s2.Ow[0], x3D[1] - s2.Ow[1], x3D[2] - s2.Ow[2]};
  const float dist2 = nmp_norm3(normal2);
  if (dist1 == 0 || dist2 == 0) return NMP_ZERO_DIST;
  if (P.farPoints && (dist1 >= P.thFarPoints || dist2 >= P.thFarPoints)) return NMP_FAR_POINT;
  const float ratioDist = dist2 / dist1;
  const float ratioOctave = P.scaleFactors[s1.octave] / P.scaleFactors[s2.octave];
  if (ratioDist * P.ratioFactor < ratioOctave || ratioDist > ratioOctave * P.ratioFactor) return NMP_SCALE;
  return made;
}

// MapPoint::UpdateNormalAndDepth for the two observations of a new point: Ow1 / Ow2 = centres of the observing cameras (either order
// of the observation map gives the same sum), OwRef = mpCurrentKeyFrame->GetCameraCenter(), the LEFT centre also on a rig;
// levelScaleFactor = mvScaleFactors[octave of kp1], lastScaleFactor = mvScaleFactors[mnScaleLevels - 1].
MORB_NMP_FN void nmp_point_fields(const float* Pos, const float* Ow1, const float* Ow2, const float* OwRef, float levelScaleFactor,
                                  float lastScaleFactor, float* normal, float* maxDistance, float* minDistance) {
  const float n1[3] = {Pos[0] - Ow1[0], Pos[1] - Ow1[1], Pos[2] - Ow1[2]};
  const float n2[3] = {Pos[0] - Ow2[0], Pos[1] - Ow2[1], Pos[2] - Ow2[2]};
  const float l1 = nmp_norm3(n1), l2 = nmp_norm3(n2);
  MORB_NMP_UNROLL
  for (int i = 0; i < 3; ++i) normal[i] = ((0.f + n1[i] / l1) + n2[i] / l2) / 2;
  const float PC[3] = {Pos[0] - OwRef[0], Pos[1] - OwRef[1], Pos[2] - OwRef[2]};
  const float dist = nmp_norm3(PC);
  *maxDistance = dist * levelScaleFactor;
  *minDistance = *maxDistance / lastScaleFactor;
}

// ComputeDistinctiveDescriptors with two observations: both medians are vDists[0.5 * (2 - 1)] = vDists[0] = 0, so BestIdx stays at the
// first entry of map<KeyFrame*, ...>, the keyframe whose POINTER orders first.  kf2OrdersFirst = std::less<KeyFrame*>()(pKF2, pKF1).
MORB_NMP_FN bool nmp_descriptor_from_kf2(int kf2OrdersFirst) { return kf2OrdersFirst != 0; }

// The gate in front of SearchForTriangulation (:454-466): true = skip this neighbour.  baseline = |Ow2 - Ow1|; not monocular:
// baseline < pKF2->mb; monocular: baseline / medianDepthKF2 < 0.01, a float quotient compared as a double.
inline bool nmp_pair_gate(bool monocular, const float* Ow1, const float* Ow2, float mb2, float medianDepthKF2) {
  const float v[3] = {Ow2[0] - Ow1[0], Ow2[1] - Ow1[1], Ow2[2] - Ow1[2]};
  const float baseline = nmp_norm3(v);
  if (!monocular) return baseline < mb2;
  const float ratioBaselineDepth = baseline / medianDepthKF2;
  return (double)ratioBaselineDepth < 0.01;
}

}  // namespace morbnmp
