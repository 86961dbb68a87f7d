// The float arithmetic that follows the bundle adjustment of Tracking::CreateInitialMapMonocular (reference src/Tracking.cc:2400-2429):
// KeyFrame::ComputeSceneMedianDepth(2) of the first keyframe (src/KeyFrame.cc:796-826), the reset test, the rescaling of the baseline and
// of every point, and MapPoint::UpdateNormalAndDepth for a point seen by exactly the two keyframes (new_map_points_math.h).  Plain C++ that
// compiles for the host and for the device: the kernel (csrc/initial_map.hip) runs it per lane, tests/native/initial_map_math_check.cc
// serially under sanitizers.
//   * InitialMapStatus: what morb_create_initial_map_monocular_batch writes to d_status;
//   * im_depth_key / im_key_depth: a float as an unsigned key of the same order (the kernel selects the median bit by bit on the keys);
//   * im_median_rank, im_median_depth (host): vDepths[(size - 1) / 2] of the sorted depths, -1 for no point;
//   * im_status, im_scale3, im_camera_centre, im_point_fields.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "new_map_points_math.h"

#if defined(__HIPCC__)
#define MORB_IM_FN __host__ __device__ __forceinline__
#else
#define MORB_IM_FN inline
#endif

namespace morbim {

// d_status: 0 = the two-view reconstruction had failed (ok == 0), nothing was done; IM_OK; or the reasons of "Wrong initialization,
// reseting..." (Tracking.cc:2407-2408) as bits: the median depth is negative (or there is no point), fewer than minTracked points
enum InitialMapStatus { IM_NOT_RUN = 0, IM_OK = 1, IM_RESET_MEDIAN = 2, IM_RESET_COUNT = 4 };

// d_stats row
enum InitialMapStat { IM_S_POINTS = 0, IM_S_ITERATIONS = 1, IM_S_TRIALS = 2, IM_S_STOP_SEEN = 3, IM_STATS_LEN = 4 };

// a < b as floats  <=>  key(a) < key(b) as unsigned (-0 orders below +0; NaNs order beyond the infinities, by sign)
MORB_IM_FN uint32_t im_depth_key(float z) {
  uint32_t u;
  memcpy(&u, &z, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
MORB_IM_FN float im_key_depth(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  float z;
  memcpy(&z, &u, 4);
  return z;
}

// ComputeSceneMedianDepth(q = 2): vDepths[(vDepths.size() - 1) / q]
MORB_IM_FN int im_median_rank(int n) { return (n - 1) / 2; }

// z of a point in the first keyframe, whose pose is the identity: Rcw.row(2).dot(x3Dw) + zcw with Rcw.row(2) = (0, 0, 1), zcw = 0
MORB_IM_FN float im_kf1_depth(const float* X) { return ((0.f * X[0] + 0.f * X[1]) + 1.f * X[2]) + 0.f; }

MORB_IM_FN int im_status(float medianDepth, int nPoints, int minTracked) {
  const int s = (medianDepth < 0 ? IM_RESET_MEDIAN : 0) | (nPoints < minTracked ? IM_RESET_COUNT : 0);
  return s ? s : IM_OK;
}

MORB_IM_FN void im_scale3(float* v, float s) { v[0] *= s; v[1] *= s; v[2] *= s; }

// Ow = Tcw.inverse().translation() = -(Rcw^T tcw) of a 3 x 4 row-major [R | t] held as R (9) then t (3)
MORB_IM_FN void im_camera_centre(const float* T12, float* Ow) {
  for (int i = 0; i < 3; ++i) Ow[i] = -((T12[i] * T12[9] + T12[3 + i] * T12[10]) + T12[6 + i] * T12[11]);
}

// UpdateNormalAndDepth of a point of the initial map: observers keyframe 1 (at the origin) and keyframe 2, reference keyframe 2, level =
// the octave of keyframe 2's keypoint.  dist2 = {mfMaxDistance, mfMinDistance}
MORB_IM_FN void im_point_fields(const float* Pos, const float* Ow2, float levelScaleFactor, float lastScaleFactor, float* normal, float* dist2) {
  const float Ow1[3] = {0.f, 0.f, 0.f};
  morbnmp::nmp_point_fields(Pos, Ow1, Ow2, Ow2, levelScaleFactor, lastScaleFactor, normal, &dist2[0], &dist2[1]);
}

// the host's form of the kernel's selection: sort, take the rank
inline float im_median_depth(const float* z, int n) {
  if (n <= 0) return -1.f;
  std::vector<float> v(z, z + n);
  std::sort(v.begin(), v.end());
  return v[(size_t)im_median_rank(n)];
}

}  // namespace morbim
